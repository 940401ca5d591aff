"""The kernels that walk a read along its CIGAR against the oracle's plain-C restatements, on generated reads (tests/read_walk_cases.py) of 1..641
bases: the candidate scan (variant.pyx:529-720) as the byte scan, the scan on 2-bit codes and the scan on packed bytes, and the read statistics
of the INFO field (vcfutils.pyx:901-1072,1300-1390) on the expanded and on the packed table.  The committed goldens stop at 161 bases and at two
trips of 64 reads; tests/test_read_walk_cases_cpu.py shows on the oracle alone that these inputs go beyond both."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_walk_cases as C  # noqa: E402

from platypus_amd.engine import Engine

pytestmark = pytest.mark.gpu

PATHS = (dict(), dict(codes=True), dict(packed=True))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scan():
    return C.scan_regions()[0]


@pytest.fixture(scope="module")
def scan_expected(scan, oracle):
    """The oracle's records per setting, computed once."""
    return {st: [oracle.variant_candidates(g["ref"], g["ref_seq_start"], g["contig_len"], g["reads"], *st) for g in scan] for st in C.SCAN_SETTINGS}


@pytest.fixture(scope="module")
def windows():
    return C.stats_windows()


def _kw(path, n_reads):
    return dict(path, gaps=C.source_gaps(n_reads)) if path.get("packed") else path


@pytest.mark.parametrize("path", PATHS, ids=("bytes", "codes", "packed"))
def test_candidate_scan_equals_the_oracle_record_for_record(eng, scan, scan_expected, path):
    """(refPos, removed, added, read index) in emission order, for every minFlank / minBaseQual / genSNPs / genIndels setting."""
    n_reads = sum(len(g["reads"]) for g in scan)
    ra, fa = C.scan_alignments(scan, 10)
    assert ra == set(range(32)) and fa == set(range(32))                            # codes_at's funnel shift at every alignment, read and reference
    for st in C.SCAN_SETTINGS:
        got = eng.candidates(scan, *st, **_kw(path, n_reads))
        for g, (a, b) in enumerate(zip(got, scan_expected[st])):
            assert a == b, (st, g, next((x, y) for x, y in zip(a + [None], b + [None]) if x != y))
        if path:
            assert eng.last_ref_irregular.cpu().numpy()[:4].tolist() == [0, 0, 0, 1]    # the region with lowercase and IUPAC bytes took the flagged byte scan
    assert sum(len(x) for x in scan_expected[C.SCAN_SETTINGS[0]]) > 4000


@pytest.mark.parametrize("path", PATHS, ids=("bytes", "codes", "packed"))
def test_a_read_with_more_records_than_its_slice_overflows_and_retries(eng, oracle, path):
    region = C.overflow_region()
    g = region[0]
    want = oracle.variant_candidates(g["ref"], g["ref_seq_start"], g["contig_len"], g["reads"], 10, 20)
    kw = _kw(path, len(g["reads"]))
    eng.candidates(region, 10, 20, max_per_read=8, retry=False, **kw)
    last = eng.last_candidates
    assert last["status"].tolist() == [0, -8, 0]                                    # PLAT_ERR_OVERFLOW for the read that needs more, and its full count
    assert last["count"].tolist() == [2, sum(x[3] == 1 for x in want), 2] and last["count"][1] > 40
    assert eng.candidates(region, 10, 20, max_per_read=8, **kw) == [want]


@pytest.mark.parametrize("packed", (False, True), ids=("bytes", "packed"))
def test_read_statistics_equal_the_oracle(eng, oracle, windows, packed):
    """The 16 counts, the per-sample counts and the MMLQ minima in read order, with 0..200 good and 0..130 bad reads per sample (up to four
    trips of 64 lanes, the MMLQ prefix carried from trip to trip and from sample to sample)."""
    n_sup = n_mmlq = 0
    for n_ind, wins in windows.items():
        n_reads = sum(len(s["good"]) + len(s["bad"]) for w in wins for s in w["samples"])
        for brw, exact in C.STATS_SETTINGS:
            got = eng.variant_read_stats(wins, brw, exact, packed=packed, gaps=C.source_gaps(n_reads) if packed else None)
            for k, (w, res) in enumerate(zip(wins, got)):
                want = C.oracle_stats(oracle, w, brw, exact)
                for v, (a, b) in enumerate(zip(res, want)):
                    assert a == b, (n_ind, k, v, brw, exact)
                    n_sup += b[0][2]; n_mmlq += len(b[3])
    assert n_sup > 4000 and n_mmlq > 2000
