"""Reads of 251 to 2000 bases on the CPU: the oracle against the reference's answers in the two wide fixtures (and the live build of the
unmodified align.c where present), and the seeded batches of tests/long_read_cases.py against what they are for -- on the generator and the
oracle alone, no device.  tests/test_gpu_long_reads.py compares the device with the oracle on the same batches."""
import os

import numpy as np
import pytest

import long_read_cases as LC
from oracle.oracle import RefAlign

DP_SWAR_MAX_QSUM = 15000                                               # dp_core.hpp
PREP_LMAX = 448                                                         # plat_align.hip: a window is staged through LDS up to this length


def windows(oracle, hb, do_flank=0):
    """Per window (scores [H, R], DPs, saturated traceback DPs)."""
    out = []
    for w in range(hb.n_windows):
        ll, sc, ndp, nsat = oracle.align_window_counting(hb.window_haps(w), int(hb.win_start[w]), int(hb.win_end[w]), int(hb.win_flank[w]),
                                                         hb.window_reads(w), do_flank=do_flank)
        out.append((sc, ndp, nsat))
    return out


@pytest.fixture(scope="module")
def ladder(oracle):
    out = {}
    for L in LC.LADDER:
        hb = LC.ladder_batch(L)
        out[L] = (hb, windows(oracle, hb))
    return out


# ---- the oracle against the reference ---------------------------------------------------------------------------------------------------
def test_oracle_equals_the_wide_dp_fixture(oracle, golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "dp_wide_cases.npz")))      # (every member inflated once)
    ref = RefAlign() if RefAlign.available() else None
    lens = g["lens"]
    assert len(lens) == 600 and set(lens.tolist()) == set(LC.LADDER)
    assert (g["score"] == LC.SATURATED).sum() >= 3 and (g["flank"] >= 0).sum() > 400
    oracle.tb_saturated()                                               # (the counter is the process's: what tests before this one left is not this test's)
    for j in range(len(lens)):
        L = int(lens[j])
        hap, read = g["haps"][j, :L + 15].tobytes(), g["reads"][j, :L].tobytes()
        q, go = g["quals"][j, :L].tobytes(), g["gos"][j, :L + 15].tobytes()
        want = int(g["score"][j])
        assert oracle.dp_score(hap, read, q, go) == want, j
        if ref is not None:
            assert ref.dp_score(hap, read, q, go) == want, j
        if want == LC.SATURATED:                                        # the reference's traceback is undefined here: nothing recorded
            assert int(g["firstpos"][j]) == -1 and str(g["ops"][j]) == ""
            continue
        fp = int(g["firstpos"][j])
        a1, a2 = LC.strings_of(str(g["ops"][j]), fp, hap, read)
        assert oracle.dp_align(hap, read, q, go) == (want, a1, a2, fp), j
        if ref is not None:
            assert ref.dp_align(hap, read, q, go) == (want, a1, a2, fp), j
        if want > 0:
            assert oracle.flank_score(L + 15, 20, q, go, fp, a1, a2) == int(g["flank"][j]), j
    assert oracle.tb_saturated() == 0                                   # (no traceback was asked of a saturated row)


def test_oracle_equals_the_wide_mapalign_fixture(oracle, golden_dir):
    cases = LC.wide_mapalign_cases(golden_dir)
    assert len(cases) == 300 and {len(c["read"]) for c in cases} == set(LC.LADDER)
    assert sum(c["doFlank"] for c in cases) >= 40 and any(c["score"] == LC.SATURATED for c in cases) and any(c["score"] == 0 for c in cases)
    assert max(len(c["hap"]) for c in cases) > 4096
    n_sat_flank = 0
    for k, c in enumerate(cases):
        oracle.tb_saturated()
        sc, _ = oracle.align_read_to_hap(c["read"].encode(), bytes(c["qual"]), c["readStart"], c["hap"].encode(), c["hapStart"], c["flank"],
                                         c["doFlank"])
        assert sc == c["score"], k
        n_sat_flank += oracle.tb_saturated() if c["doFlank"] else 0     # (with a flank the reference traces back in plain mode too: no effect there)
    assert n_sat_flank == 0                                             # the generator drew flank-mode cases until no DP saturates


@pytest.mark.skipif(not RefAlign.available(), reason="the unmodified align.c is built only where the reference tree is present")
def test_oracle_equals_the_live_reference_on_a_fresh_seed(oracle):
    ref = RefAlign()
    rng = np.random.default_rng(8128)
    B = b"ACGT"
    n_sat = 0
    for j in range(300):
        L = int(LC.LADDER[j % len(LC.LADDER)])
        hap = bytearray(rng.choice(list(B + b"N"), L + 15, p=[.245, .245, .245, .245, .02]).astype(np.uint8).tobytes())
        off = int(rng.integers(0, 16))
        read = bytearray(hap[off:off + L])
        for p in (range(L) if j % 10 == 9 else rng.integers(0, L, int(rng.integers(0, 8)))):   # every tenth row: no base is left as it was
            read[int(p)] = B[(B.find(read[int(p)]) + 1 + int(rng.integers(0, 3))) % 4]
        if j % 3 == 0:
            p, k = int(rng.integers(5, L - 15)), int(rng.integers(1, 9))
            read = read[:p] + read[p + k:] + bytearray(rng.choice(list(B), k).astype(np.uint8).tobytes())
        q = bytes(rng.integers(60 if j % 10 == 9 else 0, 94, L).astype(np.uint8).tolist())
        go = bytes([45]) * (L + 15) if j % 10 == 9 else bytes(rng.integers(1, 46, L + 15).astype(np.uint8).tolist())
        hap, read = bytes(hap), bytes(read)
        want = ref.dp_score(hap, read, q, go)
        assert oracle.dp_score(hap, read, q, go) == want, j
        if want == LC.SATURATED:
            n_sat += 1
            continue
        a = ref.dp_align(hap, read, q, go)
        assert oracle.dp_align(hap, read, q, go) == a, j
        if want > 0:
            assert oracle.flank_score(L + 15, 20, q, go, a[3], a[1], a[2]) == ref.flank_score(L + 15, 20, q, go, a[3], a[1], a[2]), j
    assert n_sat >= 1


def test_saturated_traceback_is_counted_and_reads_nothing_outside(oracle):
    """Every base substituted at quality 93, 2000 bases: the plain score is 15 872, the traceback-mode call counts itself and returns no
    alignment (align.c would start at _backpointers[-1])."""
    rng = np.random.default_rng(3)
    hap = bytes(rng.choice(list(b"AC"), 2015).astype(np.uint8))
    read = bytes(rng.choice(list(b"GT"), 2000).astype(np.uint8))
    q, go = bytes([93]) * 2000, bytes([45]) * 2015
    oracle.tb_saturated()
    assert oracle.dp_score(hap, read, q, go) == LC.SATURATED and oracle.tb_saturated() == 0
    assert oracle.dp_align(hap, read, q, go) == (LC.SATURATED, b"", b"", 0)
    assert oracle.tb_saturated() == 1 and oracle.tb_saturated() == 0


# ---- reach: the batches meet what they are for -------------------------------------------------------------------------------------------
def test_generator_is_deterministic():
    a, b = LC.ladder_batch(449), LC.ladder_batch(449)
    for f in ("hap_seq", "read_seq", "read_qual", "read_pos", "read_off", "hap_off", "read_kind", "read_flags"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_ladder_batches_reach(ladder):
    qs_above = qs_below = 0
    scores = []
    for L in LC.LADDER:
        hb, res = ladder[L]
        rl = np.diff(hb.read_off)
        assert (rl == L).all() and hb.n_windows == len(LC.LADDER_WINDOWS) <= 12
        R, Hn = np.diff(hb.win_read_begin), np.diff(hb.win_hap_begin)
        assert R.min() < 13 and R.max() > 64 and R.max() % 64 != 0      # both pair packings, a partial second group of 64 reads
        assert 8 <= R.min() and R.max() <= 75 and set(Hn.tolist()) <= {3, 4}
        assert int(hb.win_flank.max()) == min(2 * L, 2500)
        qsum = np.add.reduceat(hb.read_qual.astype(np.int64), hb.read_off[:-1])
        qs_above += int((qsum > DP_SWAR_MAX_QSUM).sum()); qs_below += int((qsum <= DP_SWAR_MAX_QSUM).sum())
        assert (qsum > DP_SWAR_MAX_QSUM).any()
        for w, (name, _) in enumerate(LC.LADDER_WINDOWS):
            sc, ndp, _ = res[w]
            if name == "tandem":                                        # several candidates: more DPs than aligned pairs
                assert ndp > int((sc >= 0).sum()), (L, w)
            if name == "hapn":
                assert any(b"N" in h for h in hb.window_haps(w))
            if name == "edge":                                          # reads at and over both haplotype ends
                rd = hb.window_reads(w)
                h0 = int(hb.win_start[w] - hb.win_flank[w])
                hl = min(len(h) for h in hb.window_haps(w))
                assert min(rd["pos"]) < h0 and max(rd["end"]) > h0 + hl
            scores.append(sc.ravel())
        rd_flags = hb.read_flags
        assert (rd_flags & 512).any()
        assert any((s == -1).any() for s, _, _ in res)
        # a good read that overlaps its window by fewer than 7 bases
        ov = np.minimum(hb.read_end, np.repeat(hb.win_end, R)) - np.maximum(hb.read_pos, np.repeat(hb.win_start, R))
        assert ((ov < 7) & (hb.read_kind == 0) & ((rd_flags & 512) == 0)).any()
        assert (hb.read_kind == 2).any()
        assert (np.array([any(np.frombuffer(s, dtype=np.uint8) == ord("N")) for w in range(hb.n_windows) for s in hb.window_reads(w)["seq"]])).any()
    allsc = np.concatenate(scores)
    assert (allsc == 0).any() and (allsc == LC.SATURATED).any()
    assert qs_above > 100 and qs_below > 100
    hl = np.concatenate([np.diff(ladder[L][0].hap_off) for L in LC.LADDER])
    assert hl.max() > 4096 and hl.min() < 4096 and hl.max() <= 16384


def test_mixed_batches_reach(oracle):
    mb = LC.mixed_batches()
    offs = set()
    for name, hb in mb.items():
        assert hb.n_windows <= 12
        offs |= set((hb.read_off[:-1] % 16).tolist())
        windows(oracle, hb)                                             # the oracle takes every window (haplotypes long enough for every read)
    assert len(offs) == 16
    lens_of = lambda hb, w: np.diff(hb.read_off)[hb.win_read_begin[w]:hb.win_read_begin[w + 1]]
    # (a) exactly one long read per window, first, last, or in the middle of the second group of 64
    hb = mb["one_long"]
    seen = set()
    for w in range(hb.n_windows):
        rl = lens_of(hb, w)
        long_ = np.flatnonzero(rl > 250)
        assert len(long_) == 1 and int(rl[long_[0]]) in (449, 600, 2000) and rl[rl <= 250].min() >= 36
        k = int(long_[0])
        where = "first" if k == 0 else "last" if k == len(rl) - 1 else "middle" if 80 <= k < 112 and len(rl) > 112 else "?"
        seen.add((int(rl[k]), where))
    assert seen >= {(449, "first"), (600, "last"), (2000, "middle"), (2000, "first"), (449, "middle"), (2000, "last")}
    # (b) longest read 448 next to longest read 449
    hb = mb["seam"]
    longest = [int(lens_of(hb, w).max()) for w in range(hb.n_windows)]
    assert PREP_LMAX in longest and PREP_LMAX + 1 in longest and longest[0] == PREP_LMAX and longest[1] == PREP_LMAX + 1
    # (c) windows of 100-base reads only, the batch's longest read 2000
    hb = mb["far_long"]
    per = [set(lens_of(hb, w).tolist()) for w in range(hb.n_windows)]
    assert per.count({100}) >= 3 and {2000} in per and np.diff(hb.win_read_begin).max() > 64
    # the reads whose ungapped proof hangs on nlow: the four mismatches of the mapping diagonal cost more than the DP finds, staged and not
    hb = mb["low_quals"]
    assert [int(lens_of(hb, w).max()) for w in range(2)] == [PREP_LMAX, PREP_LMAX + 1]
    for w, (sc, _, _) in enumerate(windows(oracle, hb)):
        rd = hb.window_reads(w)
        trap = [r for r in range(len(rd["seq"])) if len(rd["seq"][r]) == LC.TRAP_LEN and min(rd["qual"][r]) == 1]
        assert len(trap) == 8
        for r in trap:
            assert sorted(rd["qual"][r])[-4:] == [LC.TRAP_Q] * 4 and sum(q < 20 for q in rd["qual"][r]) == LC.TRAP_LEN - 4
            assert 0 < sc[0, r] < 4 * LC.TRAP_Q, (w, r, sc[0, r])
    # (d) 251 .. 513 in steps of 1
    hb = mb["steps"]
    assert hb.n_windows == 1 and sorted(lens_of(hb, 0).tolist()) == list(range(251, 514))


def test_nowhere_batch_saturates_where_it_can(oracle):
    """Random reads against random haplotypes.  A gapped path costs about 11 per base whatever the read holds (measured: scores of 3264..3436 at 300
    bases and 7750..8013 at 700), so only the 2000-base reads reach 15 872; there every pair does."""
    hb = LC.nowhere_batch()
    assert (hb.read_kind == 2).all() and hb.read_qual.min() >= 60 and hb.read_qual.max() <= 93
    res = windows(oracle, hb)
    assert [int(np.diff(hb.read_off)[hb.win_read_begin[w]]) for w in range(3)] == [300, 700, 2000]
    assert all((sc >= 0).all() for sc, _, _ in res)                     # none is skipped
    assert (res[2][0] == LC.SATURATED).all()
    assert res[0][0].min() > 2000 and res[1][0].min() > 5000


def test_flank_batches_never_saturate_a_traceback(oracle):
    """The condition under which flank mode is defined in the reference: over all of flank_batches() no traceback-mode DP returns 15 872."""
    fb = LC.flank_batches()
    assert sorted(fb) == sorted(L for L in LC.LADDER if L <= 1000) + [2000]
    n_dp = 0
    for L, hb in fb.items():
        assert (np.diff(hb.read_off) == L).all() and (hb.win_flank > 0).all()
        for sc, ndp, nsat in windows(oracle, hb, do_flank=1):
            assert nsat == 0, L
            n_dp += ndp
    assert n_dp > 10000
    # and the condition is not empty: the plain ladder does saturate tracebacks at the long end
    assert sum(nsat for sc, ndp, nsat in windows(oracle, LC.ladder_batch(2000), do_flank=1)) > 0
