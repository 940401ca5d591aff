"""The inputs of tests/test_gpu_wide_windows.py (tests/wide_window_cases.py) on the oracle alone: the windows have the haplotype counts and
the interleaving the GPU test relies on, the uploaded shapes still reach every launch branch of plat_em_window_batch, the EM really iterates
on them, and the posterior cases are neither ties nor trivial -- and the oracle's calculatePosterior, which the goldens pin at 12 haplotypes at
most, agrees with a 50-digit evaluation of the same formula at up to 100."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_window_cases as W  # noqa: E402


@pytest.mark.parametrize("n_ind,seed", W.LIKELIHOOD_BATCHES)
def test_likelihood_batches_interleave_narrow_and_wide_windows(n_ind, seed):
    hb = W.likelihood_batch(n_ind, seed)
    H = W.hap_counts(hb)
    assert hb.n_windows == W.N_WINDOWS and hb.n_ind == n_ind
    assert {2, 16, 32, 64} <= set(H.tolist()) and H.max() == 64
    waves = W.genotype_waves(hb)
    assert any(2 in w and 64 in w for w in waves)                       # a wave of k_genotype with G = 3 beside G = 2 080
    assert sum(len(set(w)) > 1 for w in waves) >= len(waves) // 2
    assert hb.n_reads < 600                                             # a handful of reads per sample and window: a few seconds of oracle time
    for h in (2, 8, 64):
        m = W.member_matrix(h)
        assert m.shape == (h, h.bit_length() - 1) and len({tuple(r) for r in m.tolist()}) == h and not m[0].any()
    assert max(s["var_in_hap"].shape[1] for s in W.window_sites(64, np.random.default_rng(0))) == 6


def test_em_shapes_reach_every_launch_branch_and_thread_count():
    got = {sh: W.em_branch(*sh) for sh in W.EM_SHAPES}
    assert got == W.EM_BRANCHES
    assert {b[:2] for b in got.values()} == {("wide", True), ("wide", False), ("narrow", True), ("narrow", False)}
    assert {b[2] for b in got.values() if b[0] == "wide"} == {64, 128, 256}
    # (the likelihood batches: 64 haplotypes with 1 sample stream in k_em_wide, with 3 samples they fall back to k_em)
    assert W.em_branch(1, 64) == ("wide", True, 256) and W.em_branch(3, 64) == ("narrow", False, 64)


@pytest.fixture(scope="module")
def em_results(oracle):
    """Per shape: the batch and the oracle's EM on it (use_em 0)."""
    out = {}
    for sh in W.EM_SHAPES:
        b = W.em_batch(*sh)
        out[sh] = (b, [oracle.em_call(b["n_reads"][w], b["gl"][w], 100, 0) for w in range(len(b["hap_counts"]))])
    return out


def test_em_batches_mix_window_sizes_and_iterate(em_results):
    iters = []
    for (n_ind, max_haps), (b, res) in em_results.items():
        counts = b["hap_counts"]
        assert 6 <= len(counts) <= 10 and max(counts) == max_haps and counts.count(max_haps) == 1 and counts[0] != max_haps
        assert {h for h in (1, 2, 7, 33) if h < max_haps} <= set(counts)
        assert (b["n_reads"].max(axis=1) > 0).all()
        if n_ind > 1:
            assert (b["n_reads"] == 0).any()
        assert all(x.shape == (n_ind, h * (h + 1) // 2) and x.max() <= 1.0 + 1e-300 for x, h in zip(b["gl"], counts))
        assert min(x.min() for x in b["gl"]) == 1e-300
        iters += [r[3] for r, h in zip(res, counts) if h == max_haps]
        assert all(np.isfinite(r[0]).all() and abs(r[0].sum() - 1) < 1e-9 for r in res)
    assert min(iters) >= 26 and max(r[3] for b, res in em_results.values() for r in res) == 100     # tens of iterations, and the cap


@pytest.fixture(scope="module")
def posterior_cases(em_results):
    """(n_reads, gl, freq, mask, prior) of every variant of every uploaded batch, frequencies from the oracle's EM."""
    rng = np.random.default_rng(99)
    cases = []
    for sh, (b, res) in em_results.items():
        for w, mask, prior in W.em_batch_variants(b, rng):
            cases.append((b["n_reads"][w], b["gl"][w], res[w][0], mask, prior))
    return cases


def test_posterior_cases_are_neither_ties_nor_trivial(posterior_cases):
    vals = [W.posterior_unrounded(*c) for c in posterior_cases]
    kept = [(v, fl) for v, fl in vals if not W.is_tie(v)]
    assert len(vals) >= 200 and 100 * (len(vals) - len(kept)) <= len(vals)                   # at most 1 case in 100 left out as a tie
    trivial = sum(round(v) == 0 or fl for v, fl in kept)
    assert 2 * trivial <= len(kept), (trivial, len(kept))
    assert len({round(v) for v, fl in kept}) > 30


def test_oracle_posterior_against_fifty_digits(posterior_cases, oracle):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    n = 0
    for n_reads, gl, freq, mask, prior in posterior_cases:
        if W.is_tie(W.posterior_unrounded(n_reads, gl, freq, mask, prior)[0]):
            continue
        H = len(freq)
        f = [mp.mpf(float(x)) for x in freq]
        fp = [mp.mpf(0) if m else x for m, x in zip(mask, f)]
        tot = mp.fsum(fp)
        if tot > 0:
            fp = [x / tot for x in fp]
        pairs = [(r, s) for r in range(H) for s in range(r, H)]
        wv = [(2 if r != s else 1) * f[r] * f[s] for r, s in pairs]
        wn = [(2 if r != s else 1) * fp[r] * fp[s] for r, s in pairs]
        lv = ln = mp.mpf(0)
        for i in np.nonzero(np.asarray(n_reads) != 0)[0]:
            row = [mp.mpf(float(x)) for x in gl[i]]
            sv, sn = mp.fdot(wv, row), mp.fdot(wn, row)
            lv += mp.log(sv) if sv > 0 else -708
            ln += mp.log(sn) if sn > 0 else -708
        ratio = mp.exp(ln - lv)
        if not ratio > mp.mpf("1e-300"):
            ratio = mp.mpf("1e-300")
        p = mp.mpf(float(prior))
        want = -10 * (mp.log10(ratio * (1 - p)) - mp.log10(p + ratio * (1 - p)))
        assert oracle.variant_posterior(n_reads, gl, freq, mask, prior) == float(mp.floor(want + mp.mpf("0.5")) if want >= 0 else mp.ceil(want - mp.mpf("0.5")))
        n += 1
    assert n >= 200
