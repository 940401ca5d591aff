"""The population kernels beyond the 12 haplotypes of the committed goldens (tests/wide_window_cases.py): windows of 2..64 haplotypes side by
side through the likelihood path (k_genotype with G = 3 beside G = 2 080 in one wave, k_haplotype_score, k_variant_posterior and
k_genotype_call at 64 haplotypes), and uploaded likelihoods of up to 100 haplotypes at every launch branch of plat_em_window_batch -- against
the oracle's restatements of cpopulation.pyx:384-594 and vcfutils.pyx:163-334.  tests/test_wide_window_cases_cpu.py checks the inputs, and the
oracle's posterior at these sizes, without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_window_cases as W  # noqa: E402
from test_gpu_parity import check_against_oracle, check_genotypes  # noqa: E402

from platypus_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _check_em(oracle, n_ind, counts, hap_begin, gl_off, n_reads, gl, use_em, freq, em, calls, iters):
    """Frequencies, EM likelihoods, calls and iteration counts of every window against the oracle's EM on the same likelihoods: only + * / in the
    reference's order, so equal doubles."""
    for w, H in enumerate(counts):
        G = H * (H + 1) // 2
        rows = gl[gl_off[w]:gl_off[w] + n_ind * G].reshape(n_ind, G)
        f, e, c, it, mc = oracle.em_call(n_reads[w], rows, 100, use_em)
        assert it == iters[w], (w, H, it, iters[w])
        assert np.array_equal(f, freq[hap_begin[w]:hap_begin[w] + H]), (w, H)
        assert c.tolist() == calls[w].tolist(), (w, H)
        live = np.asarray(n_reads[w]) > 0
        got = em[gl_off[w]:gl_off[w] + n_ind * G].reshape(n_ind, G)
        assert np.array_equal(e[live], got[live]) and not got[~live].any(), (w, H)


def _check_posteriors(eng, oracle, db, n_ind, n_reads, gl_rows, freq, hap_begin, variants):
    """variants: (window, mask, prior).  Rounded phred values equal, except where the value before round() lies within W.TIE_MARGIN of a
    half-integer (derivation of the margin: tests/wide_window_cases.py); at most 1 case in 100 may be left out for that."""
    got = eng.variant_posteriors(db, [v[0] for v in variants], [v[1] for v in variants], [v[2] for v in variants])
    kept = 0
    for k, (w, mask, prior) in enumerate(variants):
        f = freq[hap_begin[w]:hap_begin[w + 1]]
        if W.is_tie(W.posterior_unrounded(n_reads[w], gl_rows(w), f, mask, prior)[0]):
            continue
        kept += 1
        assert got[k] == oracle.variant_posterior(n_reads[w], gl_rows(w), f, mask, prior), (k, w, len(f), prior)
    assert 100 * (len(variants) - kept) <= len(variants)
    return kept


def _check_genotype_calls(eng, oracle, db, n_ind, gl_rows, gof_rows, freq, hap_begin, sites):
    res = eng.genotype_calls(db, sites)
    for s, (ph, lik, out4) in zip(sites, res):
        w = s["window"]
        f = freq[hap_begin[w]:hap_begin[w + 1]]
        for i in range(n_ind):
            oph, olik, o4 = oracle.genotype_call(f, gl_rows(w)[i], gof_rows(w)[:, i], s["var_in_hap"], s["is_ref"], n_ind)
            assert ph[i].tolist() == oph.tolist(), (w, i)
            assert np.array_equal(lik[i], olik) and np.array_equal(out4[i], o4, equal_nan=True), (w, i)
    return len(sites) * n_ind


# ---- through the likelihood path ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=W.LIKELIHOOD_BATCHES, ids=lambda p: "%d_samples" % p[0])
def called(request, eng):
    hb = W.likelihood_batch(*request.param)
    H = W.hap_counts(hb)
    assert {2, 16, 32, 64} <= set(H.tolist()) and any(2 in w and 64 in w for w in W.genotype_waves(hb))
    db = eng.upload(hb)
    st = eng.call_windows(db)
    eng.synchronize()
    return dict(hb=hb, db=db, st=st, ll=db.loglik.cpu().numpy()[:hb.n_pairs], sc=db.score.cpu().numpy()[:hb.n_pairs], gl=db.gl.cpu().numpy(),
                gof=db.gof.cpu().numpy(), n_reads=np.asarray(hb.seg_n_good).reshape(hb.n_windows, hb.n_ind))


def test_wide_windows_alignment_and_genotype_likelihoods(called, oracle):
    """Scores and per-read log-likelihoods bit for bit; logl, gl and gof within the libm tolerances of tests/test_gpu_parity.py."""
    hb = called["hb"]
    check_against_oracle(oracle, hb, called["ll"], called["sc"], called["st"])
    check_genotypes(oracle, hb, called["ll"], called["db"].logl.cpu().numpy(), called["gl"], called["gof"])


@pytest.mark.parametrize("use_em", (0, 1))
def test_wide_windows_em(called, eng, oracle, monkeypatch, use_em):
    monkeypatch.delenv("PLAT_EM_NARROW", raising=False)
    hb, db = called["hb"], called["db"]
    eng.em(db, 100, use_em)
    eng.synchronize()
    _check_em(oracle, hb.n_ind, W.hap_counts(hb), hb.win_hap_begin, hb.gl_off, called["n_reads"], called["gl"], use_em, db.freq.cpu().numpy(),
              db.em.cpu().numpy(), db.calls.cpu().numpy().reshape(hb.n_windows, hb.n_ind), db.em_iters.cpu().numpy())


def test_wide_windows_haplotype_scores(called, eng, oracle):
    """hap_like = the oracle's hap1Like on the device's own likelihoods (same doubles), HapScore = the oracle's clustering of them."""
    hb, ll = called["hb"], called["ll"]
    like, score = eng.haplotype_scores(called["db"])
    for w in range(hb.n_windows):
        h0, h1 = hb.win_hap_begin[w], hb.win_hap_begin[w + 1]
        R = hb.win_read_begin[w + 1] - hb.win_read_begin[w]
        rows = ll[hb.pair_off[w]:hb.pair_off[w] + (h1 - h0) * R].reshape(h1 - h0, R)
        ind = max(i for i in range(hb.n_ind) if hb.seg_n_good[w * hb.n_ind + i] != 0)
        s0 = hb.seg_read_begin[w * hb.n_ind + ind] - hb.win_read_begin[w]
        s1 = hb.seg_read_begin[w * hb.n_ind + ind + 1] - hb.win_read_begin[w]
        exp = []
        for h in range(h1 - h0):
            arr = np.concatenate([rows[h, s0:s1], [999.0]])
            exp.append(oracle.genotype_loglik(arr, arr, True, 1)[2])
        assert like[h0:h1].tolist() == exp, w
        assert score[w] == oracle.haplotype_score(exp), w


def test_wide_windows_posteriors_and_genotype_calls(called, eng, oracle, monkeypatch):
    monkeypatch.delenv("PLAT_EM_NARROW", raising=False)
    hb, db, gl, gof = called["hb"], called["db"], called["gl"], called["gof"]
    eng.em(db, 100, 0)
    eng.synchronize()
    freq = db.freq.cpu().numpy()
    H = W.hap_counts(hb)
    G = H * (H + 1) // 2
    gl_rows = lambda w: gl[hb.gl_off[w]:hb.gl_off[w] + hb.n_ind * G[w]].reshape(hb.n_ind, G[w])
    gof_rows = lambda w: gof[hb.gl_off[w]:hb.gl_off[w] + hb.n_ind * G[w]].reshape(G[w], hb.n_ind)
    rng = np.random.default_rng(31)
    variants, sites = [], []
    for w in range(hb.n_windows):
        m = W.member_matrix(H[w])
        for k in range(m.shape[1]):
            variants += [(w, m[:, k].astype(np.uint8), float(10.0 ** rng.uniform(-4, np.log10(0.5)))), (w, m[:, k].astype(np.uint8), 0.5)]
        sites += [dict(s, window=w) for s in W.window_sites(H[w], rng)]
    assert _check_posteriors(eng, oracle, db, hb.n_ind, called["n_reads"], gl_rows, freq, hb.win_hap_begin, variants) > 100
    assert {s["var_in_hap"].shape[1] for s in sites} == {1, 2, 3, 4, 5, 6}
    assert _check_genotype_calls(eng, oracle, db, hb.n_ind, gl_rows, gof_rows, freq, hb.win_hap_begin, sites) > 100


# ---- every launch branch of plat_em_window_batch, on uploaded likelihoods ---------------------------------------------------------------------
def test_em_shapes_still_reach_every_launch_branch():
    """The host's choice (plat_population.hip:543-566) restated in W.em_branch: all four branches, and k_em_wide at its three thread counts."""
    got = {sh: W.em_branch(*sh) for sh in W.EM_SHAPES}
    assert got == W.EM_BRANCHES
    assert {b[:2] for b in got.values()} == {("wide", True), ("wide", False), ("narrow", True), ("narrow", False)}
    assert {b[2] for b in got.values() if b[0] == "wide"} == {64, 128, 256}


@pytest.fixture(scope="module")
def uploaded(eng):
    out = {}
    for sh in W.EM_SHAPES:
        b = W.em_batch(*sh)
        out[sh] = (b, eng.upload_likelihoods(b["n_ind"], b["hap_counts"], b["n_reads"], b["gl"], b["gof"]))
    return out


@pytest.mark.parametrize("shape", W.EM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_em_launch_branches_equal_the_oracle(uploaded, eng, oracle, monkeypatch, shape):
    """Windows of 1..max_haps haplotypes in one launch: the kernels size their loops and streams by the window and carve their LDS by the batch."""
    monkeypatch.delenv("PLAT_EM_NARROW", raising=False)
    b, lb = uploaded[shape]
    n_ind, counts = b["n_ind"], b["hap_counts"]
    gl = np.concatenate([x.reshape(-1) for x in b["gl"]])
    most = 0
    for use_em in (0, 1):
        eng.em(lb, 100, use_em)
        eng.synchronize()
        iters = lb.em_iters.cpu().numpy()
        _check_em(oracle, n_ind, counts, lb.host.win_hap_begin, lb.host.gl_off, b["n_reads"], gl, use_em, lb.freq.cpu().numpy(), lb.em.cpu().numpy(),
                  lb.calls.cpu().numpy().reshape(len(counts), n_ind), iters)
        most = max(most, int(iters[:len(counts)].max()))
    assert most >= 26


@pytest.mark.parametrize("shape", W.EM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_posteriors_and_genotype_calls_on_uploaded_likelihoods(uploaded, eng, oracle, monkeypatch, shape):
    """k_variant_posterior and k_genotype_call at up to 100 haplotypes, with 25 samples or fewer and with more (the frequency-weighted rule)."""
    monkeypatch.delenv("PLAT_EM_NARROW", raising=False)
    b, lb = uploaded[shape]
    n_ind = b["n_ind"]
    eng.em(lb, 100, 0)
    eng.synchronize()
    freq = lb.freq.cpu().numpy()
    rng = np.random.default_rng(7 + 1000 * shape[0] + shape[1])
    assert _check_posteriors(eng, oracle, lb, n_ind, b["n_reads"], lambda w: b["gl"][w], freq, lb.host.win_hap_begin, W.em_batch_variants(b, rng)) >= 10
    assert _check_genotype_calls(eng, oracle, lb, n_ind, lambda w: b["gl"][w], lambda w: b["gof"][w], freq, lb.host.win_hap_begin, W.em_batch_sites(b, rng)) >= 10
