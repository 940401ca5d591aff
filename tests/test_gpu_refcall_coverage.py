"""plat_refcall_coverage_batch (Engine.refcall_coverage) against hostapi.ReadArray.countReadsCoveringRegion(p, p + 1) looped in Python as
outputRefCall loops it (variantcaller.pyx:774-784): the smallest count of a block over its samples and positions, the per-position
counts, PLAT_REFCOV_RAISES where the reference raises, PLAT_REFCOV_EMPTY for a minimum over nothing.  The shapes are the smallest at which
the kernel can go wrong: the thread stride (256) and the tile seam (1024), the staged range's edges, the switch to global memory."""
import numpy as np
import pytest

from platypus_amd import _lib, hostapi as H

pytestmark = pytest.mark.gpu

RAISES, EMPTY = _lib.PLAT_REFCOV_RAISES, _lib.PLAT_REFCOV_EMPTY


@pytest.fixture(scope="module")
def eng():
    return H.get_engine()


class _Table:
    """Samples -> one read table with a slice per sample, and the reference's counts per sample and position (computed once per position)."""

    def __init__(self, samples):
        self.pos, self.end, self.slices, self.arrays, self.memo = [], [], [], [], []
        for reads, longest in samples:
            reads = sorted(reads, key=lambda r: r[0])                    # (stable, as ReadArray's own sort)
            arr = H.ReadArray([H.AlignedRead(b"A", b"!", p, end=e) for p, e in reads])
            assert [r.pos for r in arr.array] == [p for p, _ in reads] and [r.end for r in arr.array] == [e for _, e in reads]
            if longest is not None:
                arr.longestRead = longest
            self.slices.append((len(self.pos), len(reads), arr.longestRead))
            self.pos += [p for p, _ in reads]
            self.end += [e for _, e in reads]
            self.arrays.append(arr)
            self.memo.append({})

    def count(self, s, p):
        m = self.memo[s]
        if p not in m:
            try:
                m[p] = self.arrays[s].countReadsCoveringRegion(p, p + 1)
            except RuntimeError:
                m[p] = RAISES
        return m[p]

    def expected(self, interval):
        start, end, first, ns, _ = interval
        if start >= end or ns == 0:
            return EMPTY, np.zeros(0, dtype=np.int32)
        per = np.array([min(self.count(s, p) for s in range(first, first + ns)) for p in range(start, end)], dtype=np.int32)
        return int(per.min()), per

    def check(self, eng, intervals):
        mins, counts = eng.refcall_coverage(self.pos, self.end, self.slices, intervals)
        for k, iv in enumerate(intervals):
            want_min, want = self.expected(iv)
            assert mins[k] == want_min, (k, iv, int(mins[k]), want_min)
            assert (counts[k] is None) == (not iv[4])
            if iv[4]:
                assert np.array_equal(counts[k], want), (k, iv, np.flatnonzero(counts[k] != want)[:5])
        return mins, counts


def _pile(rng, lo, hi, depth, length=150):
    n = max(1, (hi - lo) * depth // length)
    return [(int(p), int(p) + length) for p in rng.integers(lo, hi, n)]


def test_no_reads_empty_intervals_and_no_samples(eng):
    t = _Table([([], None), ([(100, 250)], None)])
    mins, counts = t.check(eng, [(10, 300, 0, 1, 1), (5, 5, 0, 1, 1), (9, 3, 0, 2, 0), (50, 400, 0, 0, 1), (10, 300, 0, 2, 1), (120, 200, 1, 1, 0)])
    assert mins.tolist() == [0, EMPTY, EMPTY, EMPTY, 0, 1] and not counts[0].any() and len(counts[0]) == 290 and len(counts[1]) == 0


@pytest.mark.parametrize("per_position", [0, 1])
def test_thread_stride_and_tile_seam(eng, per_position):
    rng = np.random.default_rng(11)
    t = _Table([(_pile(rng, 0, 4000, 30), None)])
    ivs = [(start, start + n, 0, 1, per_position) for n in (1, 255, 256, 257, 1023, 1024, 1025, 2049) for start in (0, 777)]
    mins, _ = t.check(eng, ivs)
    assert 0 < mins.max() < 60                                              # (a 30x pile: covered everywhere behind position 0 ...)
    assert t.check(eng, [(3990, 4400, 0, 1, per_position)])[0][0] == 0      # (... and not behind its end)


def test_pointer_difference_is_not_coverage(eng):
    # a 20-base read lying between two 150-base reads over the site is counted although it does not reach the site
    t = _Table([([(100, 250), (150, 170), (160, 310)], None)])
    mins, counts = t.check(eng, [(200, 201, 0, 1, 1), (100, 320, 0, 1, 1)])
    assert mins[0] == 3 and counts[0].tolist() == [3]
    # reads at position 0 are never found by the first bound (its key is at least 1): one read counted where three cover
    t = _Table([([(0, 150), (0, 100), (30, 180)], None)])
    mins, counts = t.check(eng, [(50, 51, 0, 1, 1), (0, 200, 0, 1, 1), (0, 30, 0, 1, 0)])
    assert counts[0].tolist() == [1] and mins[2] == 0


def test_longest_and_the_ends_of_the_table(eng):
    rng = np.random.default_rng(12)
    reads = _pile(rng, 500, 2500, 20, length=100)
    for longest in (None, 1000, 3000, 7):                                   # the table's own; larger than any read (also than p); shorter than the reads
        t = _Table([(reads, longest)])
        t.check(eng, [(0, 600, 0, 1, 1),                                    # p - longest < 1, then the first reads
                      (0, 400, 0, 1, 0), (100, 499, 0, 1, 1),               # wholly in front of the first read
                      (2700, 3900, 0, 1, 1), (2601, 2602, 0, 1, 0),         # wholly behind the last one: e0 == N, the walk reaches N
                      (2300, 2800, 0, 1, 1), (400, 2700, 0, 1, 0)])


def test_walk_reads_one_entry_past_the_staged_range(eng):
    # every position of [3000, 3100) has s0 == e0 == iHi == 1 < N == 2: the walk looks at end[iHi], the entry behind the staged range
    for end_at_ihi, want in ((5150, 0), (100, RAISES)):
        t = _Table([([(10, 160), (5000, end_at_ihi)], 150)])
        mins, counts = t.check(eng, [(3000, 3100, 0, 1, 1), (3000, 3100, 0, 1, 0), (20, 100, 0, 1, 1)])
        assert mins.tolist() == [want, want, 1] and set(counts[0].tolist()) == {want}


def test_malformed_read_is_a_data_verdict(eng):
    with pytest.raises(RuntimeError, match="Read start pointer"):
        H.ReadArray([H.AlignedRead(b"A", b"!", 300, end=360), H.AlignedRead(b"A", b"!", 400, end=350)]).countReadsCoveringRegion(370, 371)
    t = _Table([([(300, 360), (400, 350)], None), ([(200, 420), (310, 460)], None)])
    ivs = [(365, 380, 0, 1, 0), (365, 380, 0, 1, 1), (300, 340, 0, 1, 1), (365, 380, 1, 1, 1), (300, 500, 0, 2, 1), (365, 380, 1, 1, 0)]
    mins, counts = t.check(eng, ivs)
    assert mins.tolist() == [RAISES, RAISES, 1, 2, RAISES, 2] and RAISES in counts[1].tolist() and RAISES not in counts[3].tolist()
    assert counts[4].min() == RAISES and counts[4].max() >= 0               # canonicalised where it raises, counted where it does not


def test_pile_deeper_than_the_lds_capacity(eng):
    cap = _lib.load().plat_refcov_lds_reads()
    assert 256 <= cap <= 1 << 15
    rng = np.random.default_rng(13)
    deep = sorted((int(p), int(p) + int(n)) for p, n in zip(rng.integers(1000, 1100, cap + 300), rng.integers(120, 200, cap + 300)))
    thin = _pile(rng, 0, 3000, 10)
    t = _Table([(deep, None), (thin, None), (deep[:cap], None), (deep[:cap + 1], None)])     # ... and exactly at / one over the capacity
    ivs = [(900, 1700, 0, 1, 1), (0, 3000, 0, 1, 0), (900, 1700, 0, 2, 1), (2000, 2300, 0, 2, 0), (0, 2049, 2, 1, 1), (0, 2049, 3, 1, 1), (1100, 1200, 2, 2, 0)]
    mins, counts = t.check(eng, ivs)
    assert counts[0].max() > cap                                            # (the whole pile between the two pointers somewhere)


def test_minimum_over_samples(eng):
    rng = np.random.default_rng(14)
    a, b, c = _pile(rng, 0, 2000, 30, 150), _pile(rng, 300, 1500, 8, 76), _pile(rng, 0, 2000, 15, 250)
    t = _Table([(a, None), (b, None), (c, None)])
    assert len({s[2] for s in t.slices}) == 3
    ivs = [(100, 1300, 0, 2, 1), (100, 1300, 0, 3, 1), (100, 1300, 1, 2, 0), (0, 2300, 0, 3, 1), (400, 1400, 0, 3, 0), (400, 1400, 2, 1, 0)]
    mins, counts = t.check(eng, ivs)
    assert mins[4] <= mins[5] and (counts[1] <= counts[0]).all() and mins[1] == counts[1].min()


def test_seeded_fuzz(eng):
    rng = np.random.default_rng(2024)
    samples = []
    for _ in range(3):
        n = int(rng.integers(1900, 2100))
        samples.append(([(int(p), int(p) + int(k)) for p, k in zip(rng.integers(0, 6000, n), rng.integers(1, 301, n))], None))
    t = _Table(samples)
    ivs = []
    for _ in range(200):
        start = int(rng.integers(-40, 6300))
        length = int(rng.choice([1, 3, 40, 300, 1024, 1500, 2500])) + int(rng.integers(0, 60))
        first = int(rng.integers(0, 3))
        ivs.append((start, start + length, first, int(rng.integers(1, 4 - first)), int(rng.integers(0, 2))))
    mins, _ = t.check(eng, ivs)
    assert (mins <= 0).any() and (mins > 10).any()


def test_tile_list_with_too_few_tiles_costs_time_not_values(eng):
    rng = np.random.default_rng(15)
    t = _Table([(_pile(rng, 0, 6000, 20), None)])
    ivs = [(100, 3300, 0, 1, 1), (10, 20, 0, 1, 1), (200, 5300, 0, 1, 0)]
    want = eng.refcall_coverage(t.pos, t.end, t.slices, ivs)
    got = eng.refcall_coverage(t.pos, t.end, t.slices, ivs, tile_first=[0, 2, 3, 4])          # 2 + 1 + 1 tiles where 4 + 1 + 5 are due
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1][0], got[1][0]) and np.array_equal(want[1][1], got[1][1])
    assert [t.expected(iv)[0] for iv in ivs] == got[0].tolist()
