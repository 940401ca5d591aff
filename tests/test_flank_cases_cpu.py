"""The batches of tests/flank_cases.py on the CPU: the oracle alone, in both modes, on every batch that tests/test_gpu_flank_stress.py runs with
--calculateFlankScore=1.  No traceback-mode DP of them saturates (a condition: the reference is undefined there and the device's score
unspecified, DESIGN.md "The exception"), each batch reaches what it is for, and where the unmodified align.c is built the oracle's traceback of
every classified DP equals it.

The floors below are what the seeded builders gave when this was written, every DP at a mapping position classified (the first 4 000 of each
stress batch hold the figures of profiles/flank_stress.md); a builder that changes shows here before it shows as a weaker GPU test."""
import collections

import numpy as np
import pytest

import flank_cases as FC
from oracle.oracle import RefAlign

# pairs, and per batch the least of: pairs the two modes score differently, pairs flank mode brings to 0, windows whose DP count differs,
# DPs classified, with a gap, insertion / deletion columns in a flank, deletion runs over the left / right boundary, first-column gaps,
# mismatch columns against a haplotype N in a flank
FLOORS = {
    "adversarial":        (29340, 17048, 5168, 253, 26014, 4475, 4413, 573, 3, 0, 953, 15),
    "adversarial_gapped": (30902, 22800, 5820, 257, 29736, 14429, 19323, 11094, 107, 88, 1631, 58),
    "indel_random":       (12214, 5145, 936, 36, 10784, 8468, 163728, 140729, 176, 1803, 571, 0),
    "indel_repeat":       (10839, 4694, 1054, 45, 9215, 7076, 126676, 106634, 191, 1578, 334, 0),
    "seam":               (22830, 7798, 3274, 43, 19179, 17734, 36618, 25404, 954, 502, 1068, 5287),
}
FLOOR_KEYS = ("score_differs", "score_becomes_0", "windows_dp_differs") + FC.COUNT_KEYS


@pytest.fixture(scope="module")
def counted(oracle):
    """name -> (batch, per-window counts, the first disagreement with align.c or None): one pass of the oracle per batch."""
    ref = RefAlign() if RefAlign.available() else None
    out = {}
    for name in FC.NAMES:
        hb, err = FC.batch(name), None
        try:
            per = FC.traceback_counts(oracle, hb, ref=ref, per_window=True)
        except AssertionError as e:
            err, per = e, FC.traceback_counts(oracle, hb, per_window=True)
        out[name] = (hb, per, err)
    return out


def total(per):
    c = collections.Counter()
    for p in per:
        c.update(p)
    return c


@pytest.mark.parametrize("name", FC.NAMES)
def test_no_traceback_saturates_and_the_batch_stays_in_bounds(counted, name):
    hb, per, _ = counted[name]
    assert total(per)["saturated"] == 0
    assert hb.n_pairs <= 31000
    assert int(np.diff(hb.read_off).max()) <= 250                       # (longer reads in flank mode: tests/test_gpu_long_reads.py)
    assert (hb.win_flank > 0).all()


@pytest.mark.parametrize("name", FC.NAMES)
def test_each_batch_reaches_what_it_is_for(counted, name):
    hb, per, _ = counted[name]
    c, floor = total(per), FLOORS[name]
    print(name, {k: c[k] for k in ("pairs",) + FLOOR_KEYS})
    assert c["pairs"] == hb.n_pairs == floor[0]
    for key, least in zip(FLOOR_KEYS, floor[1:]):
        assert c[key] >= least, key
    assert c["windows_dp_differs"] >= 1 and c["score_differs"] > c["score_becomes_0"] > 0


def test_the_seam_batch_covers_every_flank_context_and_length(counted):
    hb, per, _ = counted["seam"]
    _, meta = FC.seam_batch()
    assert hb.n_windows == len(meta) == 54 and int(hb.read_qual.max()) == FC.QMAX
    nh = np.diff(hb.win_hap_begin)
    assert set(nh.tolist()) == {2, 3, 4}
    assert set(np.diff(hb.read_off).tolist()) == set(FC.LENGTHS)
    hl = np.diff(hb.hap_off)
    for w, (L, F, ctx, n_ev) in enumerate(meta):
        a, b = hb.win_hap_begin[w], hb.win_hap_begin[w + 1]
        assert int(hb.win_flank[w]) == F and (hl[a:b] >= L + 15).all() and (hl[a:b] > 2 * F).all()
    by = lambda i: {k: total(p for m, p in zip(meta, per) if m[i] == k) for k in sorted(set(m[i] for m in meta))}
    events = lambda i: {k: sum(m[3] for m in meta if m[i] == k) for k in sorted(set(m[i] for m in meta))}
    # contexts: the same events in each; a repeat moves gaps along itself, so fewer runs end up over a boundary, but some do at both
    ctx = by(2)
    assert events(2) == {"homopolymer": 2082, "random": 2082, "tandem": 2082}
    for name, gaps, left, right, differs in (("random", 6916, 775, 377, 3397), ("homopolymer", 4714, 43, 33, 1895), ("tandem", 6104, 136, 92, 2506)):
        c = ctx[name]
        assert c["with_gap"] >= gaps and c["del_runs_crossing_left"] >= left and c["del_runs_crossing_right"] >= right, name
        assert c["score_differs"] >= differs and c["windows_dp_differs"] >= 13, name
    # flanks: 1, 7, 8, 9, 40 and min(2 L, 500) = 72, 200, 500.  A slice ends at hapLen - 8, so a right flank of up to 9 bases takes no gap run, and
    # a left flank of one base holds one column: what moves there is the N exemption and the 0 that ends the candidate loop
    fl = by(1)
    assert sorted(fl) == [1, 7, 8, 9, 40, 72, 200, 500]
    for F, differs, ins_in, del_in, left, right in ((1, 12, 0, 0, 0, 0), (7, 560, 166, 594, 138, 0), (8, 475, 213, 605, 93, 0), (9, 810, 384, 721, 183, 0),
                                                     (40, 3041, 23423, 13157, 280, 215), (72, 909, 1837, 1090, 82, 80), (200, 1005, 3596, 3057, 82, 131),
                                                     (500, 986, 6999, 6180, 96, 76)):
        c = fl[F]
        got = (c["score_differs"], c["ins_cols_in_flank"], c["del_cols_in_flank"], c["del_runs_crossing_left"], c["del_runs_crossing_right"])
        print("flank", F, got)
        assert all(g >= least for g, least in zip(got, (differs, ins_in, del_in, left, right))), (F, got)
        assert c["n_mismatch_cols_in_flank"] >= 32 and c["first_column_gap"] >= 1, F
    for L, c in by(0).items():
        assert c["del_runs_crossing_left"] >= 278 and c["del_runs_crossing_right"] >= 128 and c["first_column_gap"] >= 303, L


@pytest.mark.skipif(not RefAlign.available(), reason="the unmodified align.c is built only where the reference tree is present")
def test_the_oracle_traces_back_as_the_unmodified_align_c(counted):
    """Score, both alignment strings, firstpos and calculateFlankScore of every classified DP (FC.traceback_counts asserts them one by one)."""
    for name in FC.NAMES:
        assert counted[name][2] is None, (name, counted[name][2])
        assert total(counted[name][1])["classified"] >= FLOORS[name][4]
