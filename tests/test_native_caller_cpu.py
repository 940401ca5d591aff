"""The region loop's HOST logic, end to end on the CPU: platypus_amd.caller (Python mirror of the reference's
callVariantsInRegion) and the native libplat_caller.so (platypus_amd/csrc/host) must write the same VCF record text.

No GPU here, so both run on tests/fakedev: the C ABI of include/platypus_mi355x.h implemented with the parity oracle (test
infrastructure only; the product binds the HIP library and has no CPU path).  The GPU suite repeats the comparison on the real
device (tests/test_gpu_caller.py) and checks the fake against it."""
import io

import numpy as np
import pytest

from platypus_amd import caller, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options
from platypus_amd.vcfrecords import VCF


@pytest.fixture(scope="module")
def fake():
    from tests import fakedev
    old = H._engine
    H._engine = fakedev.fake_engine()
    yield fakedev.fake_caller_lib()
    H._engine = old


def _work(regs, names, extra=None):
    fasta = H.FastaFile({r["chrom"]: r["ref"] for r in regs})
    out = []
    for k, r in enumerate(regs):
        bufs = []
        for i, reads in enumerate(r["samples"]):
            rs = [H.AlignedRead(x["seq"], x["qual"], x["pos"], x["mapq"], x["flag"], end=x["end"], cigarOps=x["cigar"], matePos=x.get("matePos", -1))
                  for x in reads]
            good, bad, broken = rs, [], []
            if extra:
                good, bad, broken = extra(k, i, rs)
            bufs.append(H.bamReadBuffer(good, bad, broken, sample=names[i]))
        out.append((r["chrom"], r["start"], r["end"], bufs))
    return fasta, out


def _both(lib, regs, names, extra=None, workers=2, per_chunk=2, **opt):
    fasta, work = _work(regs, names, extra)
    o1 = default_options(**opt)
    py = io.StringIO()
    nw = caller.callVariantsInRegions(work, fasta, o1, VCF(names), py)
    nc = F.NativeCaller(0, workers, per_chunk, lib=lib)
    o2 = default_options(**opt)
    txt = nc.call_regions([F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work], names, o2)
    st = nc.stats
    nc.close()
    assert txt.split("\n") == py.getvalue().split("\n")
    assert o1.rlen == o2.rlen and st["n_windows"] == nw and st["n_records"] == txt.count("\n")
    return txt, st


def test_native_equals_python_one_and_three_samples(fake):
    for ns, n, kw in ((1, 3, dict(region_len=4000, snp_rate=3e-3, indel_rate=1e-3, read_len=100, depth=30)),
                      (3, 2, dict(region_len=5000, snp_rate=4e-3, indel_rate=2e-3, read_len=150, depth=25))):
        regs = [synth.config4_region(10 * ns + i, n_samples=ns, **kw) for i in range(n)]
        txt, st = _both(fake, regs, ["S%d" % (i + 1) for i in range(ns)])
        assert st["n_records"] > 15 and st["n_windows_failed"] == 0


def test_native_equals_python_greedy_haplotype_filter(fake):
    """More than five variants in a window: getFilteredHaplotypes grows the best haplotypes greedily, one alignment batch per
    variant (variantFilter.pyx:440-506); coverage filter on and off, a small maxHaplotypes."""
    regs = [synth.config4_region(70 + i, n_samples=2, region_len=2500, snp_rate=8e-2, indel_rate=1e-2, read_len=100, depth=30) for i in range(2)]
    txt, st = _both(fake, regs, ["A", "B"])
    assert st["n_windows_greedy"] > 20
    txt, st = _both(fake, regs[:1], ["A", "B"], filterVarsByCoverage=0, maxVariants=12, maxHaplotypes=20)
    assert st["n_windows_greedy"] > 5


def test_native_equals_python_bad_reads_broken_mates_and_empty_samples(fake):
    """badReads and brokenMates take part in the likelihoods and the read statistics (chaplotype.pyx:341-373, vcfutils.pyx:1300-1390);
    a sample without reads in one region, a region without reads at all, regions of different read lengths (options.rlen)."""
    rng = np.random.default_rng(8)
    regs = [synth.config4_region(90 + i, n_samples=2, region_len=3000, snp_rate=4e-3, indel_rate=1.5e-3, read_len=[100, 76, 125][i], depth=40)
            for i in range(3)]
    regs.append(synth.config4_region(99, n_samples=2, region_len=1500, read_len=100, depth=20))
    regs[3]["samples"] = [[], []]

    def split(k, i, rs):
        if k == 1 and i == 1:
            return [], [], []
        good, bad, broken = [], [], []
        for r in rs:
            u = rng.random()
            if u < 0.08:
                r.mapq = int(rng.integers(0, 20)); r.bitFlag |= 512
                bad.append(r)
            elif u < 0.12:
                r.matePos = r.pos + int(rng.integers(-400, 400))
                broken.append(r)
            else:
                good.append(r)
        return good, bad, broken
    txt, st = _both(fake, regs, ["S1", "S2"], extra=split, workers=3, per_chunk=1)
    assert st["n_records"] > 20


@pytest.mark.parametrize("opt", [dict(minPosterior=0), dict(maxVariants=3, minPosterior=20), dict(mergeClusteredVariants=0, minReads=3),
                                 dict(largeWindows=1, maxVarDist=30, minVarDist=5), dict(skipDifficultWindows=1, maxVariants=4),
                                 dict(genIndels=0), dict(minVarFreq=0.2, badReadsThreshold=30, qdThreshold=30, hapScoreThreshold=1)])
def test_native_equals_python_option_variants(fake, opt):
    regs = [synth.config4_region(200 + i, n_samples=1, region_len=3000, snp_rate=1.2e-2, indel_rate=3e-3, read_len=100, depth=30) for i in range(2)]
    _both(fake, regs, ["S1"], **opt)


def test_native_many_chunks_per_worker(fake):
    """Several chunks per worker, one region per chunk, a region without reads in the middle: the same text whatever the split."""
    regs = [synth.config4_region(40 + i, n_samples=2, region_len=2500, snp_rate=4e-3, indel_rate=1e-3, read_len=100, depth=20) for i in range(7)]
    regs[3]["samples"] = [[], []]
    names = ["A", "B"]
    a, _ = _both(fake, regs, names, workers=1, per_chunk=1)
    b, _ = _both(fake, regs, names, workers=2, per_chunk=1)
    c, _ = _both(fake, regs, names, workers=2, per_chunk=3)
    assert a == b == c and a.count("\n") > 20


def test_native_refuses_what_it_does_not_build(fake):
    regs = [synth.config4_region(1, region_len=1000, read_len=100)]
    fasta, work = _work(regs, ["S1"])
    nc = F.NativeCaller(0, 1, 1, lib=fake)
    from platypus_amd._lib import PlatypusDeviceError
    for bad in (dict(getVariantsFromBAMs=0),):                              # no candidate source at all (source VCFs are not built)
        with pytest.raises(PlatypusDeviceError) as e:
            nc.call_regions([F.RegionReads.from_buffers(c, s, e_, fasta, b) for c, s, e_, b in work], ["S1"], default_options(**bad))
        assert e.value.code == -6


def _split_classes(rng):
    def split(k, i, rs):
        good, bad, broken = [], [], []
        for r in rs:
            u = rng.random()
            if u < 0.08:
                r.mapq = int(rng.integers(0, 20)); r.bitFlag |= 512 if u < 0.04 else 0
                bad.append(r)
            elif u < 0.12:
                r.matePos = r.pos + int(rng.integers(-400, 400))
                broken.append(r)
            else:
                good.append(r)
        return good, bad, broken
    return split


@pytest.mark.parametrize("opt", [dict(assemble=1), dict(assemble=1, getVariantsFromBAMs=0), dict(assemble=1, assemblyRegionSize=700, assembleBrokenPairs=1, assembleBadReads=0),
                                 dict(assemble=1, assembleAll=0), dict(assemble=1, noCycles=1, assemblerKmerSize=21)])
def test_native_equals_python_with_the_assembler(fake, opt):
    """--assemble=1 (variantcaller.pyx:496-519, 276-321; assembler.pyx:1391-1476): tiles of every region of a chunk assembled in one device
    batch, their variants join the BAM candidates (or stand alone), same text as the Python region loop -- tiling, read selection
    (badReads / brokenMates / QCFail), doWeNeedToAssembleThisRegion, sources in the INFO field."""
    rng = np.random.default_rng(12)
    regs = [synth.config4_region(700 + i, n_samples=2, region_len=2600, snp_rate=3e-3, indel_rate=2.5e-3, read_len=100, depth=30) for i in range(3)]
    regs[1]["samples"][1] = []
    txt, st = _both(fake, regs, ["S1", "S2"], extra=_split_classes(rng), workers=2, per_chunk=2, **opt)
    assert st["n_assembly_tiles"] >= (6 if opt.get("assembleAll", 1) else 0)
    if opt.get("assembleAll", 1):
        assert st["n_assembler_variants"] > 5 and "Source=Assembler" in txt or "Platypus,Assembler" in txt
    if not opt.get("getVariantsFromBAMs", 1):
        assert "Source=Platypus" not in txt and txt.count("\n") > 3


@pytest.mark.parametrize("opt", [dict(outputRefCalls=1), dict(outputRefCalls=1, refCallBlockSize=150, minPosterior=60),
                                 dict(outputRefCalls=1, refCallBlockSize=37, maxVariants=2, skipDifficultWindows=1), dict(outputRefCalls=1, assemble=1)])
def test_native_equals_python_with_reference_calls(fake, opt):
    """--outputRefCalls=1 (variantcaller.pyx:584-607,764-867; window.py:172-219): REFCALL lines for the blocks between calling windows,
    between the called positions of a window, for windows without a call and for windows the loop leaves uncalled -- the text of the
    Python region loop (itself pinned by refcall_cases / regionprep_cases and its window-by-window shape)."""
    regs = [synth.config4_region(400 + i, n_samples=2, region_len=2500, snp_rate=5e-3, indel_rate=1.5e-3, read_len=100, depth=[30, 4, 12][i % 3]) for i in range(4)]
    regs[2]["samples"][0] = []                                             # a sample without reads: blocks without coverage
    txt, st = _both(fake, regs, ["S1", "S2"], workers=2, per_chunk=2, **opt)
    assert st["n_refcall_records"] == txt.count("\tREFCALL\t") >= 20 and st["n_records"] - st["n_refcall_records"] >= 5


def test_native_equals_python_on_array_regions(fake):
    """synth.config4_region_arrays (the generator of the config-4 benchmark): arrays straight into the native loop, the same reads
    as objects into the Python loop."""
    regs = [synth.config4_region_arrays(300 + i, region_len=6000, snp_rate=3e-3, indel_rate=1e-3, n_samples=2, read_len=150, depth=30) for i in range(3)]
    names = ["S1", "S2"]
    fasta = H.FastaFile({r["chrom"]: r["ref"].tobytes() for r in regs})
    work = [(r["chrom"], r["start"], r["end"], [H.bamReadBuffer(F.aligned_reads_from_arrays(s), sample=names[i]) for i, s in enumerate(r["samples"])])
            for r in regs]
    o1, o2 = default_options(), default_options()
    py = io.StringIO()
    caller.callVariantsInRegions(work, fasta, o1, VCF(names), py)
    nc = F.NativeCaller(0, 2, 2, lib=fake)
    txt = nc.call_regions([F.region_from_arrays(r) for r in regs], names, o2)
    assert txt == py.getvalue() and txt.count("\n") > 30
    # the planted variants come back
    called = {(ln.split("\t")[0], int(ln.split("\t")[1])) for ln in txt.split("\n")[:-1]}
    snps = [(r["chrom"], p + 1) for r in regs for (p, rem, add), t0, t1 in zip(r["variants"], r["truth"][0], r["truth"][1]) if len(rem) == len(add) and t0 + t1 > 0]
    assert sum(k in called for k in snps) >= 0.9 * len(snps)


def test_reference_call_blocks_batched_equals_window_by_window(fake):
    """--outputRefCalls=1 (variantcaller.pyx:584-607,764-867): REFCALL lines for the blocks between calling windows, between the
    called positions of a window and for windows without a call; the batched shape of the Python region loop writes what the
    window-by-window shape writes."""
    regs = [synth.config4_region(400 + i, n_samples=2, region_len=2500, snp_rate=5e-3, indel_rate=1.5e-3, read_len=100, depth=[30, 4][i % 2]) for i in range(3)]
    names = ["S1", "S2"]
    fasta, work = _work(regs, names)
    for opt in (dict(outputRefCalls=1), dict(outputRefCalls=1, refCallBlockSize=150, minPosterior=60)):
        one = io.StringIO()
        for c, s_, e, bufs in _work(regs, names)[1]:
            caller.callVariantsInRegion(c, s_, e, bufs, fasta, default_options(**opt), VCF(names), one)
        many = io.StringIO()
        caller.callVariantsInRegions(_work(regs, names)[1], fasta, default_options(**opt), VCF(names), many)
        lines = many.getvalue().split("\n")[:-1]
        assert one.getvalue() == many.getvalue()
        ref = [ln for ln in lines if "\tREFCALL\t" in ln]
        var = [ln for ln in lines if "\tREFCALL\t" not in ln]
        assert len(ref) >= 20 and len(var) >= 5
        # the blocks tile the gaps: every REFCALL line carries END and Size = END - POS + 1 - 1 (0-based start, half-open end)
        for ln in ref:
            f = ln.split("\t")
            info = dict(kv.split("=") for kv in f[7].split(";"))
            assert int(info["Size"]) == int(info["END"]) - (int(f[1]) - 1) and f[4] in ("N", "T") and f[9].startswith("./.:-1,-1,-1:-1:-1:")


def test_runtime_errors_end_the_call_and_window_errors_skip_the_window(fake, monkeypatch):
    """A device error that no single window can be guilty of (HIP runtime, out of memory) in the window batch must end plat_call_regions
    with that code -- not be swallowed window by window with PLAT_OK and records missing; an input-class error is retried per window
    and only costs the windows that fail again (variantcaller.pyx:568-615)."""
    import ctypes as C
    from platypus_amd._lib import PlatypusDeviceError
    from tests import fakedev
    dev = C.CDLL(fakedev.FAKE_LIB)
    regs = [synth.config4_region(500, n_samples=1, region_len=3000, snp_rate=4e-3, indel_rate=1e-3, read_len=100, depth=30)]
    fasta, work = _work(regs, ["S1"])
    rr = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
    nc = F.NativeCaller(0, 1, 1, lib=fake)
    good = nc.call_regions(rr, ["S1"], default_options())
    assert good.count("\n") > 5 and nc.stats["n_windows_called"] == nc.stats["n_windows"]
    # syncs of a chunk: 1 = candidate scan, 2 = window batch (no greedy rounds here)
    for code in (-2, -3):                                                    # PLAT_ERR_HIP, PLAT_ERR_NOMEM
        dev.plat_fake_reset_sync_count()
        monkeypatch.setenv("PLAT_FAKE_FAIL_SYNC", "%d:2" % code)
        with pytest.raises(PlatypusDeviceError) as e:
            nc.call_regions(rr, ["S1"], default_options())
        assert e.value.code == code
    dev.plat_fake_reset_sync_count()
    monkeypatch.setenv("PLAT_FAKE_FAIL_SYNC", "-9:2")                        # PLAT_ERR_BAD_INPUT once: the retry goes through
    again = nc.call_regions(rr, ["S1"], default_options())
    assert again == good and nc.stats["n_windows_failed"] == 0 and nc.stats["n_windows_called"] == nc.stats["n_windows"]
    monkeypatch.delenv("PLAT_FAKE_FAIL_SYNC")
    nc.close()


def two_allele_regions():
    """Regions with sites where the reads show TWO alternative SNP alleles, each in the same number of reads (a tie of type, length
    and support)."""

    rng = np.random.default_rng(21)
    regs = [synth.config4_region(900 + i, n_samples=2, region_len=3000, snp_rate=2e-3, indel_rate=5e-4, read_len=100, depth=40) for i in range(4)]
    n_sites = 0
    for r in regs[:3]:                                                      # (the fourth region stays as it is: no pair, no replay)
        taken = {v[0] for v in r["variants"]}
        sites = [p for p in rng.choice(np.arange(r["start"] + 150, r["end"] - 150), size=40, replace=False).tolist()
                 if all(abs(p - q) > 12 for q in taken)][:7]
        for p in sites:
            taken.add(p)
            ref_b = r["ref"][p]
            alts = [b for b in b"ACGT" if b != ref_b]
            a1, a2 = (alts[k] for k in rng.choice(3, size=2, replace=False))
            for reads in r["samples"]:                                      # the same number of reads for either allele: a tie of support too
                cover = [x for x in reads if x["pos"] + 12 <= p < x["pos"] + len(x["seq"]) - 12 and len(x["cigar"]) == 1]
                for k, x in enumerate(cover[:2 * min(14, len(cover) // 2)]):
                    s = bytearray(x["seq"])
                    s[p - x["pos"]] = a1 if k % 2 == 0 else a2
                    x["seq"] = bytes(s)
            n_sites += 1
    return regs, n_sites


def test_sites_with_two_alternative_alleles_follow_the_python2_dictionary_order(fake):
    """Two SNP alleles at one position compare equal under Variant.__richcmp__ (refPos, type, nRemoved): `sorted` keeps them in the
    order the candidate dictionaries yield them, Python-2 dicts keyed by hash((refName, refPos, removed, added)) (variant.pyx:270-280,
    :747-751; variantcaller.pyx:457).  Both region loops replay those dictionaries for a region that holds such a pair (and only
    then); the order they arrive at differs from first-occurrence order for some of the sites below, and decides ALT / PP / FR / NF / NR
    of the records."""
    regs, n_sites = two_allele_regions()
    txt, st = _both(fake, regs, ["A", "B"])
    multi = [ln.split("\t") for ln in txt.split("\n") if ln and "," in ln.split("\t")[4]]
    assert n_sites >= 15 and len(multi) >= 3, (n_sites, len(multi))
    # the dictionary order is not the order of first occurrence: for some of the pairs the candidate list holds the alleles the other way
    # round than the reads showed them (what reaches the record text of THESE windows is then ordered by haplotype sequence,
    # mergeHaplotypes, variantcaller.pyx:325-383 -- the candidate order decides where support ties are broken: greedy haplotype
    # filter, coverage filter)
    fasta, work = _work(regs, ["A", "B"])
    cands, _ = caller.generateVariantsInRegions(work, fasta, default_options())
    flipped = pairs = 0
    for r, vs in zip(regs, cands):
        first = {}
        for x in [x for reads in r["samples"][:1] for x in reads]:
            if len(x["cigar"]) == 1:
                for v in vs:
                    if v.nAdded == 1 and v.nRemoved == 1 and x["pos"] <= v.refPos < x["pos"] + len(x["seq"]) and x["seq"][v.refPos - x["pos"]] == v.added[0]:
                        first.setdefault((v.refPos, v.added), len(first))
        for a, c in zip(vs, vs[1:]):
            if a.refPos == c.refPos and a.nAdded == c.nAdded == 1 and a.nRemoved == c.nRemoved == 1 and (a.refPos, a.added) in first and (c.refPos, c.added) in first:
                pairs += 1
                flipped += first[(a.refPos, a.added)] > first[(c.refPos, c.added)]
    assert pairs >= 12 and 0 < flipped < pairs, (pairs, flipped)
    # ... and where support ties are broken it reaches the text: with one variant per window allowed (filterVariantsByCoverage keeps the
    # best supported, the first of equals) the surviving allele of such a pair is the dictionary's first.  Native = Python there too,
    # and the native loop without its replay (a switch for this test) calls other alleles.
    top, st = _both(fake, regs, ["A", "B"], maxVariants=1)
    import os
    os.environ["PLAT_CALLER_FIRST_OCCURRENCE_ORDER"] = "1"
    try:
        nc = F.NativeCaller(0, 2, 2, lib=fake)
        plain = nc.call_regions([F.RegionReads.from_buffers(c, s_, e, fasta, b) for c, s_, e, b in work], ["A", "B"], default_options(maxVariants=1))
        nc.close()
    finally:
        os.environ.pop("PLAT_CALLER_FIRST_OCCURRENCE_ORDER")
    assert plain != top and plain.count("\n") == top.count("\n")
    os.environ["PLAT_CALLER_HOST_TALLY"] = "1"                              # the candidate tally on the host takes the same way
    try:
        nc = F.NativeCaller(0, 2, 2, lib=fake)
        assert nc.call_regions([F.RegionReads.from_buffers(c, s_, e, fasta, b) for c, s_, e, b in work], ["A", "B"], default_options(maxVariants=1)) == top
        nc.close()
    finally:
        os.environ.pop("PLAT_CALLER_HOST_TALLY")


def test_the_loaders_own_figures_for_its_tables(fake, monkeypatch):
    """plat_read_table.longest_read / most_bases (optional: what ReadArray knows of itself as reads are appended, cwindow.pyx:173-174,272): the same
    text with the figures (the tables of fastcaller.ReadTable carry them), without them (0: the library walks the arrays) -- and, with
    PLAT_CALLER_CHECK_HINTS=1, a figure that does not describe its table is refused instead of believed."""
    monkeypatch.setenv("PLAT_CALLER_CHECK_HINTS", "1")
    regs = [synth.config4_region(60 + i, n_samples=2, region_len=2500, snp_rate=4e-3, indel_rate=2e-3, read_len=100, depth=20) for i in range(3)]
    names = ["A", "B"]
    fasta, work = _work(regs, names)

    def call(edit=None):
        rr = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
        for r in rr:
            for tabs in r.samples:
                for t in tabs:
                    st = t.struct()
                    if t.n:
                        assert st.longest_read == int((t.end.astype(np.int64) - t.pos).max()) and st.most_bases == int(np.diff(t.off).max())
                    if edit:
                        edit(st)
        nc = F.NativeCaller(0, 2, 2, lib=fake)
        try:
            return nc.call_regions(rr, names, default_options())
        finally:
            nc.close()

    with_figures = call()
    assert with_figures.count("\n") > 10

    def forget(st):
        st.longest_read = 0; st.most_bases = 0
    assert call(forget) == with_figures

    def lie(st):
        if st.n_reads:
            st.longest_read += 1
    with pytest.raises(Exception):
        call(lie)


def test_a_caller_leaves_nothing_behind(tmp_path):
    """tests/caller_lifetime_driver.cpp: the whole native loop on the stand-in device as ONE program under AddressSanitizer, UBSan and LeakSanitizer (run as a
    program: nothing loads it into python).  Four callers made, used and destroyed, twice over, then the text blocks: every case writes its records, the
    second pass writes the first's text and leaves the heap where it found it, a block of more than 8 MB is gone with the last caller, and the
    sanitizers have nothing to report -- not a buffer forgotten by a worker's teardown (a leak), not one freed after its context (the stand-in's
    release calls read their context)."""
    import os
    import subprocess
    from oracle import oracle as orc
    orc.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, fake_o = str(tmp_path / "caller_lifetime_driver"), str(tmp_path / "fake_device.o")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g"] + san + ["-c", os.path.join(root, "tests", "fakedev", "fake_device.c"), "-o", fake_o])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-mavx2", "-pthread", "-ffp-contract=off"] + san + ["-static-libasan",
                           os.path.join(root, "tests", "caller_lifetime_driver.cpp"), os.path.join(root, "platypus_amd", "csrc", "host", "region_caller.cpp"),
                           os.path.join(root, "tools", "synth", "region_source.cpp"), fake_o, "-L" + os.path.join(root, "oracle"), "-lorc",
                           "-Wl,-rpath," + os.path.join(root, "oracle"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")     # (leaks are what this is about; the link order as in the drivers below)
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-3000:]
    rows = {}
    for line in out.stdout.splitlines():
        head, fields = line.split(": ")
        rows[head] = {k: int(v) for k, v in zip(fields.split()[0::2], fields.split()[1::2])}
    assert len(rows) == 10
    for k in (1, 2, 3, 4):
        one, two = rows["case %d pass 1" % k], rows["case %d pass 2" % k]
        assert one["lines"] == two["lines"] > 60 and min(one["held"], two["held"]) >= 8 << 20 and abs(two["left"]) <= 1024, (k, one, two)
    for kind in ("records", "blocks"):                                      # plat_merge_record_texts, plat_merge_region_blocks
        assert rows["text " + kind]["bytes"] > 8 << 20 and abs(rows["text " + kind]["left"]) <= 1024, rows["text " + kind]


# What each PLAT_CALLER_* switch accepts, read off the parse at every site that called getenv before host/switches.hpp took them over (file:line
# of commit 336c4c0, under platypus_amd/csrc/host/).  Per field: its value with the variable unset, "", "0", "1", "yes".
_SET_AT_ALL = (0, 1, 1, 1, 1)                                               # getenv(...) != nullptr
_BEGINS_WITH_1 = (0, 0, 0, 1, 0)                                            # e && e[0] == '1'
_NOT_BEGINNING_0 = (1, 1, 0, 1, 1)                                          # !(e && e[0] == '0')
SWITCH_TABLE = {
    "NO_CODES": {"noCodes": _SET_AT_ALL},                                   # stage_a.hpp:48
    "EXPAND": {"expand": _SET_AT_ALL},                                      # stage_a.hpp:49
    "HOST_TALLY": {"hostTally": _SET_AT_ALL},                               # stage_a.hpp:255
    "HOST_B": {"hostB": _BEGINS_WITH_1},                                    # stage_b_device.hpp:10-11
    "NO_DEVICE_REPLAY": {"noDeviceReplay": _SET_AT_ALL},                    # stage_b_device.hpp:59
    "HOST_INFO": {"hostInfo": _SET_AT_ALL},                                 # stage_cde.hpp:218
    "FIRST_OCCURRENCE_ORDER": {"firstOccurrenceOrder": _SET_AT_ALL},        # stage_b_host.hpp:144
    "EVEN_TAIL": {"evenTail": _NOT_BEGINNING_0},                            # region_caller.cpp:199
    "KEEP_SPARE": {"keepSpare": _BEGINS_WITH_1},                            # region_caller.cpp:346
    "CHECK_HINTS": {"checkHints": _BEGINS_WITH_1},                          # region_caller.cpp:165
    "NO_REFCTX": {"noRefCtx": _BEGINS_WITH_1},                              # (added with the reference context, after 336c4c0: e && e[0] == '1')
    "NO_REFPREFETCH": {"noRefPrefetch": _BEGINS_WITH_1},                    # (the same)
    "TRACE": {"trace": _SET_AT_ALL,                                         # caller_common.hpp:614, chunk.hpp:166, stage_b_host.hpp:145, region_caller.cpp:507
              "traceStages": _BEGINS_WITH_1},                               # caller_common.hpp:61-62 (traceStages)
}                                                                           # (region_caller.cpp:74, PLAT_CALLER_POLL_US, stays where the caller is made)
SWITCH_DEFAULTS = dict(noCodes=0, expand=0, hostTally=0, hostB=0, noDeviceReplay=0, hostInfo=0, firstOccurrenceOrder=0, evenTail=1, keepSpare=0, checkHints=0,
                       noRefCtx=0, noRefPrefetch=0, trace=0, traceStages=0)


def test_every_switch_parses_as_it_did_at_its_old_site(tmp_path):
    """tests/switches_driver.cpp (a stand-alone program over host/switches.hpp alone, built with -fsanitize=address,undefined) sets every variable to
    every spelling the old sites told apart and prints Switches::read(): each field follows its own variable by its own rule, and no other."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "switches_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I", os.path.join(root, "platypus_amd", "csrc"), os.path.join(root, "tests", "switches_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (as tests/test_bgzf_cpu.py: a library loaded in front of ASan's runtime is no error)
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        head, fields = line.split(": ")
        got[tuple(head.split(" "))] = {k: int(v) for k, v in (f.split("=") for f in fields.split())}
    want = {}
    for name, rules in SWITCH_TABLE.items():
        for k, spelling in enumerate(("unset", "empty", "0", "1", "yes")):
            want[(name, spelling)] = dict(SWITCH_DEFAULTS, **{field: rule[k] for field, rule in rules.items()})
    assert len(SWITCH_TABLE) == 13 and len(want) == 65 and set(f for r in SWITCH_TABLE.values() for f in r) == set(SWITCH_DEFAULTS)
    assert got == want


# The device library's PLAT_* switches (platypus_amd/csrc/switches.hpp), each by the rule its own getenv site applied at commit 223080b (file:line under
# platypus_amd/csrc/).  Per field: its value with the variable unset and set to "", "0", "1", "yes", "7", "-3", "33", "2000000", "512", "256", "768", "255", "257".
DEVICE_SPELLINGS = ("unset", "empty", "0", "1", "yes", "7", "-3", "33", "2000000", "512", "256", "768", "255", "257")
_D_SET_AT_ALL = (0,) + (1,) * 13                                            # getenv(...) != nullptr
_D_BEGINS_WITH_1 = (0, 0, 0, 1) + (0,) * 10                                 # e && e[0] == '1'
_D_NOT_BEGINNING_0 = (1, 1, 0) + (1,) * 11                                  # !(e && e[0] == '0')
DEVICE_SWITCH_TABLE = {
    "PLAT_NO_UNGAPPED": {"noUngapped": _D_BEGINS_WITH_1},                   # plat_align.hip:1981-1982
    "PLAT_NO_EXACT": {"noExact": _D_BEGINS_WITH_1},                         # plat_align.hip:1983-1984
    "PLAT_NO_NLOW": {"noNlow": _D_BEGINS_WITH_1},                           # plat_align.hip:1986,1989
    "PLAT_UNGAPPED_BIGQ": {"ungappedBigq": _D_BEGINS_WITH_1},               # plat_align.hip:1987,1989
    "PLAT_SEED_XCD": {"seedXcd": _D_NOT_BEGINNING_0},                       # plat_align.hip:1819-1820, 1964-1965
    "PLAT_SLOW_GROUP": {"slowGroup": (8, 8, 8, 1, 8, 7, 8, 8, 8, 8, 8, 8, 8, 8)},                 # plat_align.hip:1811: atoi in 1..32 (SLOW_GROUP), else 8
    "PLAT_SLOW_WAVES": {"slowWaves": (4, 4, 4, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4)},                 # plat_align.hip:1813: atoi in 1..4 (SLOW_WAVES), else 4
    "PLAT_SLOW_TIMING": {"slowTiming": _D_SET_AT_ALL},                      # plat_align.hip:1844-1845
    "PLAT_SEED_DEBUG": {"seedDebug": (0, 0, 0, 0, 0, 0, 512, 0, 0, 512, 0, 512, 0, 0)},           # plat_align.hip:1985,1990,2083: atoi & 0x300 then, & 0x200 since bit 256
    #                                                                         (the sweeps alone) is retired; -3 = ...11111101 has bit 512, 2000000 = 0x1E8480 has not
    "PLAT_DP_GRID_PER_CU": {"dpGridPerCu": (8, 8, 8, 1, 8, 7, 8, 33, 2000000, 512, 256, 768, 255, 257)},   # plat_align.hip:2034: atoi > 0, else 8
    "PLAT_TB_SLAB": {"tbSlab": (0, 0, 0, 0, 0, 0, 0, 0, 2000128, 512, 256, 768, 0, 512)},   # atoi >= 256 rounded up to a multiple of 256, else 0 = not
    #                                                                         given (the 6 GiB rule); the variable came after that commit, with this rule
    "PLAT_ASM_TIMING": {"asmTiming": _D_SET_AT_ALL},                        # plat_assemble.hip:1877
    "PLAT_ASM_DEBUG": {"asmDebug": (0, 0, 0, 0, 0, 4, 12, 0, 0, 0, 0, 0, 12, 0)},                  # plat_assemble.hip:1879: atoi then, & 12 since bits 1 and 2 (the
    #                                                                         reads pass without events / probes) are retired; 7 -> 4, -3 = ...11111101 -> 12, 2000000 = 0x1E8480 -> 0
    "PLAT_ASM_WG_PER_CU": {"asmWgPerCu": (0, 0, 0, 1, 0, 7, 0, 33, 2000000, 512, 256, 768, 255, 257)},     # plat_assemble.hip:1885: atoi > 0 overrides; 0 = not given
    "PLAT_ASM_NO_KEEP": {"asmNoKeep": _D_SET_AT_ALL},                       # plat_assemble.hip:1897
    "PLAT_EM_NARROW": {"emNarrow": _D_SET_AT_ALL},                          # plat_population.hip:549
    "PLAT_SYNC_SPIN": {"syncSpin": _D_BEGINS_WITH_1},                       # plat_ctx.hip:242
    "PLAT_SYNC_POLL_US": {"syncPollNs": (-1, 0, 0, 1000, 0, 7000, -1, 33000, 2000000000, 512000, 256000, 768000, 255000, 257000)},   # plat_ctx.hip:243: atol; negative or unset = not
}                                                                           #                                                  given (-1), else x 1000 ns
DEVICE_SWITCH_DEFAULTS = dict(noUngapped=0, noExact=0, noNlow=0, ungappedBigq=0, seedXcd=1, slowGroup=8, slowWaves=4, slowTiming=0, seedDebug=0, dpGridPerCu=8, tbSlab=0,
                              asmTiming=0, asmDebug=0, asmWgPerCu=0, asmNoKeep=0, emNarrow=0, syncSpin=0, syncPollNs=-1)


def test_every_device_switch_parses_as_it_did_at_its_old_site(tmp_path):
    """tests/device_switches_driver.cpp (a stand-alone program over csrc/switches.hpp alone, built with -fsanitize=address,undefined) sets every variable
    of the device library to every spelling and prints the four read()s: each field follows its own variable by its old site's rule, and no other field
    moves.  The retired variables (PLAT_DP_IMPL, PLAT_DP_TILES, PLAT_ASM_STATIC, PLAT_ASM_FUSED=0; PLAT_SEED_DEBUG's bit 256 and PLAT_ASM_DEBUG's bits 1
    and 2 in the table above) move nothing.  A poll
    interval splits into seconds and nanoseconds below a second, the total kept."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "device_switches_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I", os.path.join(root, "platypus_amd", "csrc"), os.path.join(root, "tests", "device_switches_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (as above)
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got, polls = {}, {}
    for line in out.stdout.splitlines():
        head, fields = line.split(": ")
        vals = {k: int(v) for k, v in (f.split("=") for f in fields.split())}
        if head.startswith("poll "):
            polls[int(head.split(" ")[1])] = vals
        else:
            got[tuple(head.split(" "))] = vals
    want = {("RETIRED", "set"): dict(DEVICE_SWITCH_DEFAULTS)}
    for name, rules in DEVICE_SWITCH_TABLE.items():
        for k, spelling in enumerate(DEVICE_SPELLINGS):
            want[(name, spelling)] = dict(DEVICE_SWITCH_DEFAULTS, **{field: rule[k] for field, rule in rules.items()})
    assert len(DEVICE_SWITCH_TABLE) == 18 and len(want) == 18 * 14 + 1
    assert set(f for r in DEVICE_SWITCH_TABLE.values() for f in r) == set(DEVICE_SWITCH_DEFAULTS)
    assert all(len(rule) == len(DEVICE_SPELLINGS) for r in DEVICE_SWITCH_TABLE.values() for rule in r.values())
    assert got == want
    assert polls == {0: dict(sec=0, nsec=0), 40: dict(sec=0, nsec=40000), 999999: dict(sec=0, nsec=999999000), 1000000: dict(sec=1, nsec=0),
                     2000000: dict(sec=2, nsec=0)}
    for us, ts in polls.items():
        assert 0 <= ts["nsec"] < 10 ** 9 and ts["sec"] * 10 ** 9 + ts["nsec"] == us * 1000


def test_getenv_is_called_in_the_switch_tables_only():
    """Under platypus_amd/csrc, getenv( occurs in the two switch tables and at the one PLAT_CALLER_POLL_US site of host/region_caller.cpp, nowhere else:
    no .hip file reads the environment itself."""
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "platypus_amd", "csrc")
    sites = {}
    for d, dirs, files in os.walk(root):
        dirs[:] = [x for x in dirs if x != "build"]
        for f in files:
            if not f.endswith((".hip", ".hpp", ".h", ".cpp", ".c", ".cc", ".inc")):
                continue
            with open(os.path.join(d, f), errors="replace") as fh:
                lines = [ln for ln in fh if "getenv(" in ln]
            if lines:
                sites[os.path.relpath(os.path.join(d, f), root)] = lines
    assert set(sites) == {"switches.hpp", os.path.join("host", "switches.hpp"), os.path.join("host", "region_caller.cpp")}
    assert len(sites[os.path.join("host", "region_caller.cpp")]) == 1 and "PLAT_CALLER_POLL_US" in sites[os.path.join("host", "region_caller.cpp")][0]
