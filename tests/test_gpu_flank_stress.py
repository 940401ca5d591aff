"""--calculateFlankScore=1 on the device (dp_forward_tb and tb_flank_score of dp_traceback.hpp in k_dp_tb_jobs, the slab loop of align_impl,
select_best on flank-reduced scores) against the oracle, on the stress batches that pin the plain path and on the seam batch of
tests/flank_cases.py: events at every offset around both flank boundaries, in random sequence, homopolymers and tandem repeats.
tests/test_flank_cases_cpu.py holds, without a device, that no traceback of these batches saturates and what each of them contains.

Scores and log-likelihoods bit for bit and the reference's DP count, through both entry points; the pairs that the option changes counted
against the oracle's own count; PLAT_NO_EXACT=1; and the slab loop's later trips (PLAT_TB_SLAB=256 / 768: by default one slab holds more than
a million jobs and no batch of the suite reaches a second).  profiles/flank_stress.md has the counts, the times and which value-only change
to the traceback path each of these tests catches."""
import time

import numpy as np
import pytest

import flank_cases as FC
from test_gpu_parity import check_against_oracle, eng, oracle_windows, run_align  # noqa: F401  (eng: the module's fixture)
from test_gpu_seed_indels import _with_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(oracle):
    """name -> (the oracle's windows in flank mode, its plain scores in pair order): computed once per batch, changed by nobody."""
    cache = {}

    def get(name):
        if name not in cache:
            hb = FC.batch(name)
            plain = np.concatenate([osc.reshape(-1) for _, osc, _ in oracle_windows(oracle, hb)])
            cache[name] = (oracle_windows(oracle, hb, do_flank=1), plain)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def default_run(eng):
    """name -> (log-likelihoods, scores, stats) of the synchronous entry point in flank mode with no switch set."""
    cache = {}

    def get(name):
        if name not in cache:
            db, st, ll, sc = run_align(eng, FC.batch(name), do_flank=1)
            cache[name] = (ll.copy(), sc.copy(), st)
        return cache[name]
    return get


def _async(eng, hb):
    db = eng.upload(hb)
    eng.align_async(db, calc_flank_score=1)
    eng.synchronize()
    return db.loglik.cpu().numpy()[:hb.n_pairs], db.score.cpu().numpy()[:hb.n_pairs]


@pytest.mark.parametrize("name", FC.NAMES)
def test_flank_mode_equals_the_oracle_through_both_entry_points(eng, oracle, expected, default_run, name):
    hb = FC.batch(name)
    t0 = time.perf_counter()
    ll, sc, st = default_run(name)
    t1 = time.perf_counter()
    check_against_oracle(oracle, hb, ll, sc, st, do_flank=1, windows=expected(name)[0])
    all_, asc = _async(eng, hb)
    assert np.array_equal(asc, sc) and np.array_equal(all_, ll)
    print("%s: %d pairs, n_dp_launched %d, n_dp_reference %d, n_seed_fallback %d, synchronous call with upload %.3f s" % (
        name, hb.n_pairs, st.n_dp_launched, st.n_dp_reference, st.n_seed_fallback, t1 - t0))


@pytest.mark.parametrize("name", FC.NAMES)
def test_the_option_changes_the_pairs_the_oracle_says_it_changes(eng, expected, default_run, name):
    """Not vacuous: the plain run differs from the flank run in as many pairs as the oracle's two modes do (thousands, the count is the
    oracle's), and in the same ones."""
    hb = FC.batch(name)
    flank, plain = expected(name)
    oflank = np.concatenate([osc.reshape(-1) for _, osc, _ in flank])
    want = int((oflank != plain).sum())
    sc0 = run_align(eng, hb)[3]
    sc1 = default_run(name)[1]
    print("%s: the option changes %d of %d scores, %d of them to 0" % (name, want, hb.n_pairs, int(((oflank == 0) & (plain != 0)).sum())))
    assert want >= 4000 and int((sc1 != sc0).sum()) == want
    assert np.array_equal(sc1 != sc0, oflank != plain)
    assert (sc1 <= sc0).all()


@pytest.mark.parametrize("name", FC.NAMES)
def test_the_exact_match_switch_changes_no_flank_score(eng, default_run, name):
    """PLAT_NO_EXACT=1: the pairs that k_pairs finishes as exact matches go through the traceback DP and come out as 0 there too."""
    hb = FC.batch(name)
    ll, sc, st = default_run(name)
    db, st1, ll1, sc1 = _with_env({"PLAT_NO_EXACT": "1"}, lambda: run_align(eng, hb, do_flank=1))
    assert np.array_equal(sc1, sc) and np.array_equal(ll1, ll)
    assert int(st1.n_dp_reference) == int(st.n_dp_reference) and int(st1.n_dp_launched) >= int(st.n_dp_launched)


@pytest.mark.parametrize("slab", [256, 768])
@pytest.mark.parametrize("name", ["seam", "indel_repeat"])
def test_later_trips_of_the_slab_loop(eng, oracle, expected, default_run, name, slab):
    """PLAT_TB_SLAB: the job list in slabs of 256 / 768 jobs, so that j0 > 0 and the last slab is a partial one.  Both entry points (the
    asynchronous one walks npairs + extra_cap slots, most of its last slabs past the list's end) equal the default run and the oracle."""
    hb = FC.batch(name)
    ll, sc, st = default_run(name)
    db, st1, ll1, sc1 = _with_env({"PLAT_TB_SLAB": str(slab)}, lambda: run_align(eng, hb, do_flank=1))
    n = int(st1.n_dp_launched)
    print("%s, slab %d: n_dp_launched %d = %d full slabs + %d jobs" % (name, slab, n, n // slab, n % slab))
    assert n == int(st.n_dp_launched)
    assert -(-n // slab) >= 3 and n % slab != 0
    assert np.array_equal(sc1, sc) and np.array_equal(ll1, ll)
    check_against_oracle(oracle, hb, ll1, sc1, st1, do_flank=1, windows=expected(name)[0])
    all_, asc = _with_env({"PLAT_TB_SLAB": str(slab)}, lambda: _async(eng, hb))
    assert np.array_equal(asc, sc) and np.array_equal(all_, ll)
