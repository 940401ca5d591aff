"""Seeded inputs for the population kernels (plat_population.hip, plat_genotype.hip) beyond the 12 haplotypes of the committed goldens: windows
of 2..64 haplotypes through the likelihood path, and uploaded genotype likelihoods of up to 100 haplotypes at every launch branch of
plat_em_window_batch.  Plain Python and numpy: tests/test_wide_window_cases_cpu.py checks the inputs on the oracle alone,
tests/test_gpu_wide_windows.py compares the device with the oracle on them."""
import numpy as np

from platypus_amd import synth

# ---- through the likelihood path ------------------------------------------------------------------------------------------------------------
N_WINDOWS = 24
LIKELIHOOD_BATCHES = ((1, 6108), (3, 6101))                             # (samples, seed)


def likelihood_batch(n_ind, seed):
    """1..6 SNPs per window, every combination a haplotype: 2..64 haplotypes, 3..2 080 genotypes.  The cluster is wide enough for six SNPs
    at minVarDist (9) from one another; the depth keeps a window at a handful of reads per sample."""
    return synth.make_snp_windows(N_WINDOWS, seed, read_len=100, depth=5, n_ind=n_ind, max_snps=6, cluster=60)


def hap_counts(hb):
    return np.diff(hb.win_hap_begin).astype(int)


def genotype_waves(hb):
    """Haplotype counts of the four (window, individual) units that share a wave of k_genotype, wave by wave."""
    H = np.repeat(hap_counts(hb), hb.n_ind)
    return [tuple(H[k:k + 4].tolist()) for k in range(0, len(H), 4)]


def member_matrix(H):
    """var in haplotype, [H][log2 H]: haplotype c of make_snp_windows carries SNP k where bit k of c is set."""
    n = int(H).bit_length() - 1
    return ((np.arange(H)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)


def window_sites(H, rng):
    """Sites of one window for computeGenotypeCallAndLikelihoods: all its variants together (1..6), and each alone."""
    m = member_matrix(H)
    sets = [list(range(m.shape[1]))] + ([[k] for k in range(m.shape[1])] if m.shape[1] > 1 else [])
    if m.shape[1] > 2:
        sets.append(sorted(rng.choice(m.shape[1], 2, replace=False).tolist()))
    return [dict(var_in_hap=m[:, s], is_ref=(m[:, s].sum(axis=1) == 0).astype(np.int32)) for s in sets]


# ---- every launch branch of plat_em_window_batch, on uploaded likelihoods ---------------------------------------------------------------------
# (samples, most haplotypes of a window): the branch each reaches is worked out by em_branch() below and asserted in both test files
EM_SHAPES = ((1, 10), (1, 15), (1, 50), (3, 20), (4, 50), (100, 10), (8, 40), (100, 11), (5, 50), (100, 12), (1, 100))
EM_BRANCHES = {(1, 10): ("wide", True, 64), (1, 15): ("wide", True, 128), (1, 50): ("wide", True, 256), (3, 20): ("wide", True, 256),
               (4, 50): ("wide", False, 256), (100, 10): ("wide", False, 256),
               (8, 40): ("narrow", True, 64), (100, 11): ("narrow", True, 64),
               (5, 50): ("narrow", False, 64), (100, 12): ("narrow", False, 64), (1, 100): ("narrow", False, 64)}
LDS_GFX950 = 160 * 1024                                                 # what a workgroup may ask for on gfx950


def em_branch(n_ind, max_haps, lds_dev=LDS_GFX950):
    """The launch plat_em_window_batch chooses (plat_population.hip:543-566), restated: ("wide", M-step streams, threads) for k_em_wide,
    ("narrow", responsibilities in LDS, 64) for k_em.  If the thresholds there move, EM_SHAPES has to move with them."""
    max_g = max_haps * (max_haps + 1) // 2
    csr_bytes = n_ind * max_g * 8
    wide = max_haps * 8 + 2 * csr_bytes + n_ind * 12 + max_g * 4 + 64
    if wide <= 96 * 1024 and wide <= lds_dev and max_haps < 32768:
        pairs = n_ind * max_g
        threads = 256 if pairs > 128 else (128 if pairs > 64 else 64)
        streams = max_haps * ((n_ind * (max_haps + 1) + 7) & ~7) * 8
        return "wide", wide + streams <= 150 * 1024 and wide + streams <= lds_dev, threads
    lds = max_haps * 8 + 16
    return "narrow", n_ind >= 8 and lds + csr_bytes <= 60 * 1024 and lds + csr_bytes <= lds_dev, 64


def em_batch(n_ind, max_haps, seed=None):
    """6..10 windows of uploaded likelihoods: one with max_haps haplotypes (not the first), the others with fewer -- 1, 2, 7 and 33 among them
    where they fit -- so that the kernel sizes its streams by the window and carves its LDS by the batch.  Rows rng.random() ** 4 + 1e-300, 2 % of
    the values 1e-300; a tenth of the samples without reads where there are several.  Returns dict(n_ind, hap_counts, n_reads [nW][n_ind],
    gl [nW] of [n_ind][G], gof [nW] of [G][n_ind])."""
    rng = np.random.default_rng(1000 * n_ind + max_haps if seed is None else seed)
    n_win = int(rng.integers(6, 11))
    small = [h for h in (7, 1, 2, 33) if h < max_haps]
    counts = small[:1] + [max_haps] + small[1:]
    while len(counts) < n_win:
        counts.append(int(rng.integers(1, max_haps)) if max_haps > 1 else 1)
    n_reads = rng.integers(1, 40, (len(counts), n_ind)).astype(np.int32)
    if n_ind > 1:
        n_reads[rng.random(n_reads.shape) < 0.1] = 0
        n_reads[np.arange(len(counts)), rng.integers(0, n_ind, len(counts))] = 5       # (never a window without any reads: the reference divides by their count)
    gl, gof = [], []
    for h in counts:
        g = h * (h + 1) // 2
        x = rng.random((n_ind, g)) ** 4 + 1e-300
        x[rng.random(x.shape) < 0.02] = 1e-300
        gl.append(x)
        gof.append(rng.random((g, n_ind)) * 50)
    return dict(n_ind=n_ind, hap_counts=counts, n_reads=n_reads, gl=gl, gof=gof)


def em_batch_variants(batch, rng, per_window=3):
    """Variants for calculatePosterior on a batch: (window, 0/1 per haplotype, prior).  The masks are drawn per haplotype, and where there
    are two haplotypes or more the variant is on some and not on others (on all or on none it gives the saturated value or 0 whatever the
    likelihoods say).  Priors: the flat 0.5 for a third, else 1e-4 .. 0.5."""
    out = []
    for w, h in enumerate(batch["hap_counts"]):
        for k in range(per_window if h > 1 else 1):
            mask = (rng.random(h) < rng.uniform(0.2, 0.8)).astype(np.uint8)
            if h > 1:
                c = int(rng.integers(0, h))
                mask[c], mask[(c + 1) % h] = 1, 0
            out.append((w, mask, 0.5 if k % 3 == 0 else float(10.0 ** rng.uniform(-4, np.log10(0.5)))))
    return out


def em_batch_sites(batch, rng):
    """Sites for computeGenotypeCallAndLikelihoods on a batch: 1..3 variants drawn per haplotype, haplotype 0 the reference."""
    out = []
    for w, h in enumerate(batch["hap_counts"]):
        for n_var in {1, int(rng.integers(2, 4))}:
            m = (rng.random((h, n_var)) < 0.4).astype(np.int32)
            m[0, :] = 0
            out.append(dict(window=w, var_in_hap=m, is_ref=(m.sum(axis=1) == 0).astype(np.int32)))
    return out


# ---- calculatePosterior before its round() ----------------------------------------------------------------------------------------------------
TIE_MARGIN = 1e-6
# The posterior is round() of a value that went through log, exp and log10 of the device libm.  A few ulp per log, over at most 100 samples with
# |log| <= 708, is at most about 2e-11 relative in `ratio`, under 1e-10 in the phred value: a value further than 1e-6 from k + 0.5 rounds the
# same way on either side, with four orders of magnitude to spare.


def posterior_unrounded(n_reads, gl, freq, mask, prior):
    """Population.calculatePosterior (cpopulation.pyx:509-594) in float64 numpy without the final round(): (value, ratio was floored at 1e-300)."""
    gl, freq = np.asarray(gl, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    H = len(freq)
    r, s = np.triu_indices(H)                                           # genotype order: (r, s >= r), r outermost
    fp = np.where(np.asarray(mask) != 0, 0.0, freq)
    if fp.sum() > 0:
        fp = fp / fp.sum()
    factor = np.where(r != s, 2.0, 1.0)
    live = np.asarray(n_reads) != 0
    sv = gl[live] @ (factor * freq[r] * freq[s])
    sn = gl[live] @ (factor * fp[r] * fp[s])
    with np.errstate(divide="ignore"):
        lv = np.where(sv > 0, np.log(np.where(sv > 0, sv, 1.0)), -708.0).sum()
        ln = np.where(sn > 0, np.log(np.where(sn > 0, sn, 1.0)), -708.0).sum()
    with np.errstate(over="ignore"):
        ratio = np.exp(ln - lv)
    floored = not ratio > 1e-300
    if floored:
        ratio = 1e-300
    with np.errstate(divide="ignore"):
        return float(-10.0 * (np.log10(ratio * (1.0 - prior)) - np.log10(prior + ratio * (1.0 - prior)))), floored


def is_tie(value):
    """Within TIE_MARGIN of a half-integer (or not finite): left out of the comparison of rounded values."""
    return not np.isfinite(value) or abs(value - np.floor(value) - 0.5) < TIE_MARGIN
