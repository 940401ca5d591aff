"""plat_align_window_batch, its asynchronous twin and plat_dp_batch on reads of 251 to 2000 bases (tests/long_read_cases.py), against the
reference's answers in the two wide fixtures and against the oracle: the lengths at which k_pairs hands a read to the exact vote of k_seed_slow
(above 256), at which k_prep_reads stops staging a window through LDS (longest read above 448), and at which the scratch sizes that follow the
batch's longest read (LDS image, diagonal counters, traceback rows) leave what the other tests run.  Everything is bit-exact.

Measured on an MI355X: profiles/long_reads.md."""
import io
import os

import numpy as np
import pytest

import long_read_cases as LC
from platypus_amd import _lib, synth
from platypus_amd.batch import HostBatch
from test_gpu_parity import check_against_oracle, eng, oracle_windows, run_align, single_pair_batch  # noqa: F401  (eng: the module's fixture)

pytestmark = pytest.mark.gpu


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def _async_equals(eng, hb, ll, sc, do_flank=0):
    db = eng.upload(hb)
    eng.align_async(db, calc_flank_score=do_flank)                     # (the upload's hints are exact)
    eng.synchronize()
    assert np.array_equal(db.loglik.cpu().numpy()[:hb.n_pairs], ll) and np.array_equal(db.score.cpu().numpy()[:hb.n_pairs], sc)


# ---- 1: the reference's own answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_flank", [0, 1])
def test_wide_mapalign_golden_vectors(eng, golden_dir, do_flank):
    """mapAndAlignReadToHaplotype on reads of every LADDER length, one read per window: each case is staged or not by its own length."""
    cases = [c for c in LC.wide_mapalign_cases(golden_dir) if c["doFlank"] == do_flank]
    assert len(cases) >= (40 if do_flank else 200)
    hb = single_pair_batch(cases)
    db, st, ll, sc = run_align(eng, hb, do_flank)
    exp = np.array([c["score"] for c in cases], dtype=np.int32)
    assert np.array_equal(sc, exp), np.flatnonzero(sc != exp)[:10]
    assert st.n_dp_launched >= (sc > 0).sum() and st.n_pairs == len(cases)
    print("mapalign_wide do_flank=%d: %d pairs, %d through k_seed_slow, %d DPs, %d saturated" % (
        do_flank, len(cases), st.n_seed_fallback, st.n_dp_launched, int((sc == LC.SATURATED).sum())))


# ---- 2: the ladder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LC.LADDER)
def test_ladder_equals_the_oracle_through_both_entry_points(eng, oracle, L):
    hb = LC.ladder_batch(L)
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)
    if L > 256:
        assert st.n_seed_fallback > 0
    _async_equals(eng, hb, ll, sc)
    print("ladder L=%d: %d pairs, %d aligned, %d through k_seed_slow, %d DPs launched, %d reference DPs, %d saturated, windows %s" % (
        L, hb.n_pairs, st.n_pairs_aligned, st.n_seed_fallback, st.n_dp_launched, st.n_dp_reference, int((sc == LC.SATURATED).sum()),
        "staged" if L <= 448 else "not staged"))


# ---- 3: long and short reads in one window, one batch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_long", "seam", "far_long", "steps", "low_quals"])
def test_mixed_batches_equal_the_oracle_with_and_without_shortcuts(eng, oracle, name):
    """The short reads of a window that is not staged take k_pairs' exact-match and ungapped shortcuts on the qsum / qmin / nlow the byte loop
    computed: with the shortcuts switched off the same pairs go through the DP and every array stays what it was."""
    hb = LC.mixed_batches()[name]
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)
    _async_equals(eng, hb, ll, sc)
    db1, st1, ll1, sc1 = _with_env({"PLAT_NO_UNGAPPED": "1"}, lambda: run_align(eng, hb))
    db2, st2, ll2, sc2 = _with_env({"PLAT_NO_UNGAPPED": "1", "PLAT_NO_EXACT": "1"}, lambda: run_align(eng, hb))
    assert np.array_equal(sc1, sc) and np.array_equal(ll1, ll) and np.array_equal(sc2, sc) and np.array_equal(ll2, ll)
    print("mixed %s: %d pairs, %d through k_seed_slow, DPs launched %d / %d without the ungapped proof / %d without the exact match too" % (
        name, hb.n_pairs, st.n_seed_fallback, st.n_dp_launched, st1.n_dp_launched, st2.n_dp_launched))
    if name != "steps":                                                # (every read of `steps` has more than 256 bases: no shortcut applies)
        assert int(st.n_dp_launched) < int(st1.n_dp_launched) < int(st2.n_dp_launched)
    assert int(st.n_dp_reference) == int(st1.n_dp_reference) == int(st2.n_dp_reference)


# ---- 4: flank mode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [L for L in LC.LADDER if L <= 1000] + [2000])
def test_flank_batches_equal_the_oracle(eng, oracle, L):
    """--calculateFlankScore on windows in which no DP saturates (tests/test_long_read_cases_cpu.py proves that on the oracle): the device
    traceback over 2 (L + 8) rows and calculateFlankScore."""
    hb = LC.flank_batches(only=L)[L]
    db, st, ll, sc = run_align(eng, hb, do_flank=1)
    check_against_oracle(oracle, hb, ll, sc, st, do_flank=1)
    _async_equals(eng, hb, ll, sc, do_flank=1)


# ---- 5: reads that belong nowhere -------------------------------------------------------------------------------------------------------
def test_nowhere_batch_equals_the_oracle(eng, oracle):
    """Random reads of 300, 700 and 2000 bases at qualities 60..93.  Every pair of the 2000-base window scores 15 872; a gapped path costs about
    11 per base, so the 300- and 700-base reads end at 3264..3436 and 7750..8013 (oracle = reference) and are pinned to those values."""
    hb = LC.nowhere_batch()
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)
    a, b = hb.pair_off[2], hb.pair_off[3]
    assert (sc[a:b] == LC.SATURATED).all() and (sc >= 0).all()
    _async_equals(eng, hb, ll, sc)


# ---- 6: the DP alone ----------------------------------------------------------------------------------------------------------------------
def test_dp_wide_golden_vectors_bit_exact(eng, golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "dp_wide_cases.npz")))
    got = eng.dp_batch(g["haps"], g["reads"], g["quals"], g["gos"], g["lens"])
    assert np.array_equal(got, g["score"]), np.flatnonzero(got != g["score"])[:10]


def _dp_fuzz_rows():
    rng = np.random.default_rng(4243)
    n, lmax = 256, 2000
    lens = rng.integers(251, lmax + 1, n).astype(np.int32)
    lens[:len(LC.LADDER)] = LC.LADDER
    haps = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), (n, lmax + 15), p=[.24, .24, .24, .24, .04])
    reads = np.empty((n, lmax), dtype=np.uint8)
    for j in range(n):
        off = int(rng.integers(0, 16))
        seg = haps[j, off:off + lmax]
        reads[j, :len(seg)] = seg
        reads[j, len(seg):] = ord("A")
    mut = rng.random((n, lmax)) < 0.03
    reads[mut] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), int(mut.sum()))
    for j in range(0, n, 3):          # indels
        L = int(lens[j]); p = int(rng.integers(1, L - 2)); k = int(rng.integers(1, 9))
        reads[j, p:lmax - k] = reads[j, p + k:lmax].copy()
    quals = rng.integers(0, 94, (n, lmax)).astype(np.uint8)
    quals[rng.random((n, lmax)) < 0.1] = 0
    quals[1::4] = np.minimum(quals[1::4], 20)                          # quality sums on both sides of DP_SWAR_MAX_QSUM
    gos = rng.integers(1, 46, (n, lmax + 15)).astype(np.uint8)
    other = np.zeros(256, dtype=np.uint8)                              # every eighth row: no base is its haplotype's, high qualities, dear gaps
    other[list(b"ACGTN")] = list(b"CGTAA")
    reads[::8] = other[haps[::8, 3:lmax + 3]]
    quals[::8] = rng.integers(80, 94, (n // 8, lmax)).astype(np.uint8)
    gos[::8] = 45
    return haps, reads, quals, gos, lens


def test_dp_fuzz_vs_oracle_up_to_2000_bases(eng, oracle):
    haps, reads, quals, gos, lens = _dp_fuzz_rows()
    got = eng.dp_batch(haps, reads, quals, gos, lens)
    exp = oracle.dp_batch(haps, reads, quals, gos, lens)
    assert np.array_equal(got, exp)
    assert (exp == LC.SATURATED).any() and (exp < 2000).any()


# ---- 7: the contract at the ends ----------------------------------------------------------------------------------------------------------
def _one_window(hap, reads, flank=500):
    """reads: (bases, position, kind).  Window [flank, len(hap) - flank), quality 30."""
    rl = np.array([len(r[0]) for r in reads], dtype=np.int64)
    nR = len(reads)
    pos = np.array([r[1] for r in reads], dtype=np.int32)
    return HostBatch(
        n_ind=1, win_hap_begin=np.array([0, 1], dtype=np.int32), win_read_begin=np.array([0, nR], dtype=np.int32),
        win_start=np.array([flank], dtype=np.int32), win_end=np.array([len(hap) - flank], dtype=np.int32),
        win_flank=np.array([flank], dtype=np.int32), hap_seq=hap, hap_off=np.array([0, len(hap)], dtype=np.int64),
        read_seq=np.concatenate([r[0] for r in reads]), read_qual=np.full(int(rl.sum()), 30, dtype=np.uint8),
        read_off=np.concatenate([[0], np.cumsum(rl)]).astype(np.int64), read_pos=pos, read_end=pos + rl.astype(np.int32),
        read_mapq=np.full(nR, 60, dtype=np.uint8), read_flags=np.zeros(nR, dtype=np.int32),
        read_kind=np.array([r[2] for r in reads], dtype=np.uint8), seg_read_begin=np.array([0, nR], dtype=np.int32),
        seg_n_good=np.array([sum(r[2] == 0 for r in reads)], dtype=np.int32))


@pytest.mark.parametrize("n_reads", [1, 3])
def test_few_reads_of_more_than_4096_bases(eng, oracle, n_reads):
    """k_prep_reads' byte loop finds a thread's read by a multiply-shift whose 32-bit product wrapped for a group of few reads longer than 4096
    bases (1025 groups of 4 bases x 2^22 / reads): the loop then read outside the blob.  4101 bases is the shortest read that got there."""
    rng = np.random.default_rng(9)
    B = np.frombuffer(b"ACGT", dtype=np.uint8)
    hap = B[rng.integers(0, 4, 6000)]
    reads = []
    for k in range(n_reads):
        s = hap[900 + 7 * k:900 + 7 * k + 4101].copy()
        s[[5, 2000 + k, 4100]] = ord("N")
        reads.append((s, 900 + 7 * k, 0))
    hb = _one_window(hap, reads)
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)
    assert (sc > 0).all()


def test_read_length_contract_at_the_ends(eng, oracle):
    """k_validate takes reads of up to 32 767 bases (cAlignedRead.rlen is a short).  A haplotype has at most 16 384 bases and a pair is aligned
    only when the haplotype has the read's length + 15, so a read above 16 369 bases is never aligned: it is skipped by the overlap rule like
    any other, or the batch is PLAT_ERR_HAP_TOO_SHORT.  The scratch that follows the longest read (tile, planes, the vote's diagonal
    counters) is sized for it all the same; where the counters of a 16 384-base haplotype and the batch's longest read do not fit LDS -- from
    26 221 bases on -- the host refuses the batch with PLAT_ERR_HAP_TOO_LONG before any seeding kernel is launched."""
    rng = np.random.default_rng(6)
    B = np.frombuffer(b"ACGT", dtype=np.uint8)
    hap = B[rng.integers(0, 4, 1000)]
    far = B[rng.integers(0, 4, 32767)]
    near = hap[450:650].copy(); near[100] = ord("N")
    # a 32 767-base read outside the window is skipped, the 200-base read next to it is aligned as ever (not staged, counters for 33 767 diagonals)
    hb = _one_window(hap, [(far, 5000, 0), (near, 450, 0)], flank=400)
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)
    assert sc.tolist()[0] == -1 and sc.tolist()[1] >= 0
    # the same read as a mate (never skipped): the haplotype is shorter than the read + 15
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        eng.align(eng.upload(_one_window(hap, [(far, 0, 2), (near, 450, 0)], flank=400)))
    assert e.value.code == -5
    # 32 768 bases
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        eng.align(eng.upload(_one_window(hap, [(np.concatenate([far, far[:1]]), 5000, 0), (near, 450, 0)], flank=400)))
    assert e.value.code == -9
    # the largest haplotype: a longest read of 26 220 bases fits (dynamic + static LDS = 160 KB to the byte), one of 26 221 does not
    big = B[rng.integers(0, 4, 16384)]
    near = big[8000:8250].copy(); near[17] = ord("T") if near[17] != ord("T") else ord("G")
    hb = _one_window(big, [(far[:26220], 40000, 0), (near, 8000, 0)])
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        eng.align(eng.upload(_one_window(big, [(far[:26221], 40000, 0), (near, 8000, 0)])))
    assert e.value.code == -4
    # and the context is as good as new
    hb = synth.config1()
    db, st, ll, sc = run_align(eng, hb)
    check_against_oracle(oracle, hb, ll, sc, st)


# ---- 8: the region loops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len", [300, 500])
def test_native_region_loop_equals_python_region_loop_on_long_reads(read_len):
    from platypus_amd import caller, fastcaller as F
    from platypus_amd.options import default_options
    from platypus_amd.vcfrecords import VCF
    from test_gpu_caller import _array_regions
    regs, names, fasta, work = _array_regions(2, 1, region_len=2500, snp_rate=3e-3, indel_rate=8e-4, read_len=read_len, depth=20)
    py = io.StringIO()
    nw = caller.callVariantsInRegions(work, fasta, default_options(), VCF(names), py)
    nc = F.NativeCaller(0, 2, 1)
    txt = nc.call_regions([F.region_from_arrays(r) for r in regs], names, default_options())
    assert txt == py.getvalue() and nc.stats["n_windows"] == nw and txt.count("\n") >= 4
