"""k_pairs' seeding proof on windows whose haplotypes differ by insertions and deletions: reads over such a site match on two diagonals, reads
right of it on a neighbour of their mapping offset.  The proof (the Lemma over a set of tried diagonals, plat_align.hip "The seeding stage") must
leave every score where the reference has it, and the queue of the exact vote (n_seed_fallback) nearly empty on a random reference.

Measured on an MI355X with these batches: random reference, 12 214 pairs, n_seed_fallback 504 by default and 5 306 with PLAT_SEED_ONE_DIAG=1,
12 536 DPs either way; repeats at the site, 10 839 pairs, 947 and 8 158, 13 218 DPs (profiles/r13_seed_neighbours.md)."""
import os

import numpy as np
import pytest

from test_gpu_parity import check_against_oracle, eng, run_align  # noqa: F401  (eng: the module's fixture)

pytestmark = pytest.mark.gpu

B = b"ACGT"


def _indel_batch(seed, n_windows, repeat):
    """Windows of 2..6 haplotypes that differ by one indel of 1..20 bases each (and SNPs) at a site inside the window; repeat: the site lies in a
    homopolymer or a tandem repeat of unit 2..6 and the indel is a piece of it.  Reads of 36..250 bases from every haplotype, the site at their
    midpoint, within 10 bases of either end, or anywhere.  A third of the windows have a short flank: their reads start at haplotype offsets
    below 16 (negative neighbours) and end within L + 15 of the haplotype's end (the proven diagonal is no candidate: ncand = 0)."""
    from platypus_amd import hostapi as H
    rng = np.random.default_rng(seed)
    rnd = lambda n: bytes(rng.choice(list(B), n).astype(np.uint8))
    sub = lambda c: B[(B.index(c) + 1 + int(rng.integers(0, 3))) % 4]
    specs = []
    for w in range(n_windows):
        L = int(rng.choice([36, 76, 100, 150, 250]))
        edge = w % 3 == 0
        buf = L // 3 if edge else min(2 * L, 500)
        W = int(rng.integers(L // 3 + 40, L // 3 + 100)) if edge else int(rng.integers(20, 80))
        ref = bytearray(rnd(W + 2 * buf))
        site = buf + int(rng.integers(2, W - 2))
        unit, k = b"", 0
        if repeat:
            unit, k = rnd(int(rng.choice([1, 1, 2, 3, 4, 6]))), int(rng.integers(12, 40))
            a = max(site - k // 2, 1)
            ref[a:a + k] = (unit * k)[:k]
            ref = ref[:W + 2 * buf]
        ref = bytes(ref)
        haps, shift = [ref], [0]                                 # shift: haplotype offset minus reference offset right of the site
        for _ in range(int(rng.integers(1, 6))):
            n = int(rng.integers(1, 21))
            if rng.random() < 0.5:
                ins = (bytes(ref[site:site + n]) if n <= k // 2 else (unit * n)[:n]) if repeat else rnd(n)
                h, s = bytearray(ref[:site] + ins + ref[site:]), n
            else:
                h, s = bytearray(ref[:site] + ref[site + n:]), -n
            for _ in range(int(rng.integers(0, 3))):
                p = buf + int(rng.integers(0, max(W - 21, 1)))
                h[p] = sub(h[p])
            if bytes(h) not in haps and len(h) >= L + 15:
                haps.append(bytes(h)); shift.append(s)
        ws = 5000
        reads = []
        for _ in range(int(rng.integers(20, 40))):
            j = int(rng.integers(0, len(haps)))
            src = haps[j]
            mode = int(rng.integers(0, 6 if edge else 4))
            off = (site - L // 2 if mode == 0 else site - int(rng.integers(1, 11)) if mode == 1 else site - L + int(rng.integers(1, 11)) if mode == 2
                   else int(rng.integers(0, 16)) if mode == 4 else len(src) - L - int(rng.integers(0, 19)) if mode == 5
                   else int(rng.integers(buf - L + 8, buf + W - 8)))
            off = min(max(off, 0), len(src) - L)
            refoff = off if off <= site else max(off - shift[j], site)     # where a mapper puts the read's first base
            if not (refoff < buf + W - 7 and refoff + L > buf + 7):
                continue
            seq = bytearray(src[off:off + L])
            for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2]))):
                p = int(rng.integers(0, L))
                seq[p] = sub(seq[p])
            q = np.clip(rng.normal(34, 6, L), 2, 41).astype(np.uint8)
            reads.append(H.AlignedRead(bytes(seq), bytes(q.tolist()), ws - buf + refoff, 60, 3))
        if not reads:
            continue
        bufs = [H.bamReadBuffer(reads)]
        bufs[0].setWindowPointers(ws, ws + W)
        specs.append((haps, ws, ws + W, buf, bufs))
    return H._pack_windows(specs)


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def runs(eng):
    """Both batches through the synchronous entry point, with the default rule and with PLAT_SEED_ONE_DIAG=1."""
    out = {}
    for name, hb in (("random", _indel_batch(31, 100, False)), ("repeat", _indel_batch(32, 100, True))):
        res = {}
        for mode, env in (("default", {}), ("one", {"PLAT_SEED_ONE_DIAG": "1"})):
            db, st, ll, sc = _with_env(env, lambda: run_align(eng, hb))
            res[mode] = (ll.copy(), sc.copy(), st)
        out[name] = (hb, res)
    return out


@pytest.mark.parametrize("name", ["random", "repeat"])
def test_indel_windows_equal_the_oracle_through_both_entry_points(eng, oracle, runs, name):
    hb, res = runs[name]
    assert hb.n_windows >= 90 and 2 <= np.diff(hb.win_hap_begin).min() and np.diff(hb.win_hap_begin).max() <= 6
    ll, sc, st = res["default"]
    check_against_oracle(oracle, hb, ll, sc, st)
    db = eng.upload(hb)
    eng.align_async(db)
    eng.synchronize()
    assert np.array_equal(db.loglik.cpu().numpy()[:hb.n_pairs], ll) and np.array_equal(db.score.cpu().numpy()[:hb.n_pairs], sc)


@pytest.mark.parametrize("name", ["random", "repeat"])
def test_the_one_diagonal_switch_changes_no_result(runs, name):
    """The former rule gives the same scores and log-likelihoods and runs the same number of DPs: a pair only the Lemma proves leaves the jobs the
    exact vote would have left."""
    hb, res = runs[name]
    (ll, sc, st), (ll1, sc1, st1) = res["default"], res["one"]
    assert np.array_equal(sc, sc1) and np.array_equal(ll, ll1)
    assert int(st.n_dp_launched) == int(st1.n_dp_launched)
    assert int(st.n_dp_reference) == int(st1.n_dp_reference)


def test_the_queue_of_the_exact_vote_on_a_random_reference(runs):
    """With the former rule the reads over an indel queue for the exact vote; the Lemma over the neighbour diagonals leaves a quarter of them at the
    most (the model of tests/test_seed_bound_cpu.py: only ties of the vote stay)."""
    for name in ("random", "repeat"):
        hb, res = runs[name]
        print("%s reference: %d pairs, n_seed_fallback %d by default, %d with PLAT_SEED_ONE_DIAG=1, %d DPs" % (
            name, hb.n_pairs, res["default"][2].n_seed_fallback, res["one"][2].n_seed_fallback, res["default"][2].n_dp_launched))
    hb, res = runs["random"]
    new, old = int(res["default"][2].n_seed_fallback), int(res["one"][2].n_seed_fallback)
    assert old > 0
    assert 4 * new <= old
