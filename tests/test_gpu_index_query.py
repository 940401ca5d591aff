"""GPU tests of the index query on the device: plat_index_query_batch against the chunk lists the reference's ti_iter_query returned (the
fixture, tests/golden/index_query_cases.json.gz) and against the rule's Python statement (platypus_amd.tabixindex, which
tests/test_index_query_cpu.py pins to the reference and to the host twin) on hand-made indexes sized to where the kernels change path;
which queries are handed over; the capacity contract; the refusals; and through the caller library: whole source files in place of fetch
structures, the region loop, and an index the library wrote itself read back with no Python index code in the loop."""
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth, tabixindex
from platypus_amd.options import default_options
from tests import index_query_cases as Q, tabix_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return H.get_engine()


@pytest.fixture(scope="module")
def hand():
    """[(label, index, queries, the mirror's answers, gathered counts)]: computed once."""
    return [(label, h, qs, [h.query(*q) for q in qs], [Q.gathered_of(h, *q) for q in qs]) for label, h, qs in Q.hand_cases()]


def expect(got, want, gathered):
    """The device's answer to queries whose mirror answers and gathered counts are given: handed over exactly above the limit."""
    assert got["guard_intact"] and got["status"][0] == 0
    handed = [k for k, c in enumerate(got["count"]) if c == _lib.IDXQ_HANDED_OVER]
    assert handed == [k for k, g in enumerate(gathered) if g > Q.MAX_CHUNKS]
    for k, (w, g) in enumerate(zip(want, gathered)):
        if k in handed:
            assert got["chunks"][k] is None
            continue
        assert got["chunks"][k] == w, k
        assert got["count"][k] == (-1 if w is None else len(w)) and got["gathered"][k] == g
    live = [w for k, w in enumerate(want) if w is not None and k not in handed]
    assert got["status"][1:] == [-1, sum(len(w) for w in live), sum(gathered), len(handed), sum(w is None for w in want)]
    assert got["first"][-1] == got["status"][2]


def test_fixture_on_the_device(eng):
    """The recorded lists, file by file in one batch each: both paths (up to 64 gathered chunks, above), nothing handed over."""
    for f in Q.golden_files():
        idx = tabixindex.TabixIndex(f["tbi"])
        tables = eng.index_tables(Q.flat_of(idx))
        qs = [(q["tid"], q["beg"], q["end"]) for q in f["queries"]]
        gathered = [Q.gathered_of(idx, *q) for q in qs]
        assert max(gathered) <= Q.MAX_CHUNKS and any(g > 64 for g in gathered) and any(0 < g <= 64 for g in gathered)
        got = eng.index_query(tables, qs)
        expect(got, [q["chunks"] for q in f["queries"]], gathered)
        assert got["status"][4] == 0


def test_older_goldens_on_the_device(eng):
    for f in T.golden_files():
        idx = tabixindex.TabixIndex(f["tbi"])
        qs = [(q["tid"], q["beg"], q["end"]) for q in f["queries"]]
        got = eng.index_query(eng.index_tables(Q.flat_of(idx)), qs)
        expect(got, [idx.query(*q) for q in qs], [Q.gathered_of(idx, *q) for q in qs])
        assert got["status"][4] == 0


def test_hand_made_indexes_in_one_batch_each(eng, hand):
    seen_handed = 0
    for label, h, qs, want, gathered in hand:
        got = eng.index_query(eng.index_tables(Q.flat_of(h)), qs, cap_chunks=sum(len(w) for w in want if w is not None) + 3)
        expect(got, want, gathered)
        seen_handed += got["status"][4]
    assert seen_handed == sum(x > Q.MAX_CHUNKS for _, _, _, _, g in hand for x in g) == 2      # (one chunk beyond the limit; 4673 bins queried whole)


def test_hand_made_indexes_one_query_per_batch(eng, hand):
    for label, h, qs, want, gathered in hand:
        tables = eng.index_tables(Q.flat_of(h))
        for q, w, g in zip(qs, want, gathered):
            expect(eng.index_query(tables, [q]), [w], [g])


def test_as_bai_and_all_cases_in_one_index(eng, hand):
    """Every hand-made reference side by side in ONE index (read back from its .bai bytes), every query in one batch."""
    bins, lin, qs, want, gathered = [], [], [], [], []
    for label, h, q, w, g in hand:
        qs += [(t + len(bins), b, e) for t, b, e in q]
        want += w
        gathered += g
        bins += h.bins
        lin += h.linear
    bai = tabixindex.BamIndex(Q.Hand(bins, lin, pseudo=(0, 3), n_no_coor=5).bai())
    assert bai.bins == bins
    expect(eng.index_query(eng.index_tables(Q.flat_of(bai)), qs, cap_chunks=sum(len(w) for w in want if w is not None)), want, gathered)


def test_capacity_and_refusals(eng, hand):
    f = Q.golden_files()[0]
    idx = tabixindex.TabixIndex(f["tbi"])
    flat = Q.flat_of(idx)
    tables = eng.index_tables(flat)
    qs = [(q["tid"], q["beg"], q["end"]) for q in f["queries"]]
    want = [q["chunks"] for q in f["queries"]]
    total = sum(len(w) for w in want if w is not None)
    full = eng.index_query(tables, qs, cap_chunks=total)
    expect(full, want, [Q.gathered_of(idx, *q) for q in qs])
    for cap in (total - 1, 1, 0):
        got = eng.index_query(tables, qs, cap_chunks=cap)                       # full counts, no chunk written
        assert got["guard_intact"] and got["status"][0] == -8 and got["status"][1:] == full["status"][1:]
        assert got["count"] == full["count"] and got["first"] == full["first"] and got["chunks"] is None
    # a tid outside the index: the lowest such query, nothing else written
    got = eng.index_query(tables, qs + [(3, 0, 10), (0, 0, 10), (-1, 0, 10)])
    assert got["guard_intact"] and got["status"] == [-1, len(qs), 0, 0, 0, 0]
    # tables that break their contract: sizes that do not match the offsets, bin ids that do not ascend
    n_ref, n_bins, n_chunks, n_lin = tables["sizes"]
    for sizes in ((n_ref, n_bins - 1, n_chunks, n_lin), (n_ref, n_bins, n_chunks - 1, n_lin), (n_ref, n_bins, n_chunks, n_lin - 1), (n_ref - 1, n_bins, n_chunks, n_lin)):
        got = eng.index_query(tables, qs[:3], sizes=sizes)
        assert got["guard_intact"] and got["status"] == [-1, -1, 0, 0, 0, 0], sizes
    swapped = dict(flat, bin_id=[flat["bin_id"][1], flat["bin_id"][0]] + flat["bin_id"][2:])
    got = eng.index_query(eng.index_tables(swapped), qs[:3])
    assert got["guard_intact"] and got["status"] == [-1, -1, 0, 0, 0, 0]
    # no queries at all
    got = eng.index_query(tables, [])
    assert got["guard_intact"] and got["status"] == [0, -1, 0, 0, 0, 0] and got["first"] == [0]


def test_caller_library_queries_regrows_and_hands_over(monkeypatch, hand):
    monkeypatch.delenv("PLAT_CALLER_HOST_INDEX", raising=False)
    nc = F.NativeCaller(0, 1, 1)
    try:
        # the fixture through plat_index_open (BGZF bytes as on disk) and plat_index_query
        for f in Q.golden_files():
            idx = nc.open_index(f["tbi"])
            qs = [(q["tid"], q["beg"], q["end"]) for q in f["queries"]]
            got, info = nc.query_index(idx, qs, info=True)
            assert got == [q["chunks"] for q in f["queries"]]
            assert info["handed_over"] == 0 and info["device_calls"] in (1, 2) and info["chunks"] == sum(len(c) for c in got if c is not None)
            # many copies of one query: more chunks than the first guess of the capacity; the regrow is invisible
            big = max(range(len(qs)), key=lambda k: len(got[k] or ()))
            copies = 1024 // (len(got[big]) - 16) + 2                          # (the first guess is 16 chunks a query + 1024)
            many, info = nc.query_index(idx, [qs[big]] * copies, info=True)
            assert many == [got[big]] * copies and info["device_calls"] == 2 and len(got[big]) * copies > 16 * copies + 1024
            monkeypatch.setenv("PLAT_CALLER_HOST_INDEX", "1")
            assert nc.query_index(idx, qs) == got
            monkeypatch.delenv("PLAT_CALLER_HOST_INDEX")
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.query_index(idx, qs[:2] + [(idx.n_refs, 0, 5)])
            assert e.value.code == -1 and "query 2" in str(e.value)
            assert nc.query_index(idx, qs[:2]) == got[:2]
            idx.close()
        # hand-made indexes as .tbi and as .bai; the query beyond the limit comes back from the host twin
        handed = 0
        for label, h, qs, want, gathered in hand:
            for kind, raw in (("tbi", h.tbi()), ("bai", h.bai())):
                idx = nc.open_index(raw, kind)
                got, info = nc.query_index(idx, qs, info=True)
                assert got == want, (label, kind)
                assert info["handed_over"] == sum(g > Q.MAX_CHUNKS for g in gathered)
                handed += info["handed_over"]
                idx.close()
        assert handed == 4                                                   # (the two queries beyond the limit, as .tbi and as .bai)
    finally:
        nc.close()


def test_set_source_files_gives_the_golden_lines(monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_INDEX", raising=False)
    monkeypatch.delenv("PLAT_CALLER_HOST_TABIX", raising=False)
    nc = F.NativeCaller(0, 1, 1)
    try:
        for f in T.golden_files():
            idx = nc.open_index(f["tbi"])
            regions = [(f["names"][q["tid"]], q["beg"], q["end"]) for q in f["queries"]] + [(b"nope", 0, 100), (f["names"][0], 50, 10)]
            nc.set_source_files([(f["vcf_gz"], idx)], regions)
            got = nc.source_lines_set(len(regions))
            assert got == [b"".join(l + b"\n" for l in q["lines"]) for q in f["queries"]] + [b"", b""], f["label"]
            tf = tabixindex.TabixFile(f["vcf_gz"], f["tbi"])
            fetched = tf.fetch_blocks_batch(regions, nc, idx)                    # ... and the Python reader's batch entry point
            assert [None if b is None else b[:3] for b in fetched] == [None if b is None else b[:3] for b in (tf.fetch_blocks(*r) for r in regions)]
            nc.set_source_blocks([[b] if b is not None else [] for b in fetched])
            assert nc.source_lines_set(len(regions)) == got
            idx.close()
    finally:
        nc.close()


def test_config4_with_source_files_writes_what_source_blocks_write():
    cli = T.golden_cli()
    regs = [synth.config4_region_arrays(i, region_len=4000, n_samples=1, read_len=150) for i in range(2)]
    nc = F.NativeCaller(0, 2, 2)
    try:
        tf = tabixindex.TabixFile(cli["vcf_gz"], cli["tbi"])
        blocks = [[b for b in [tf.fetch_blocks(r["chrom"], r["start"], r["end"])] if b is not None] for r in regs]
        want = nc.call_regions([F.region_from_arrays(r) for r in regs], ["S1"], default_options(), source_blocks=blocks)
        n_lines = nc.stats["n_source_lines"]
        assert n_lines > 0 and "File" in want
        idx = nc.open_index(cli["tbi"])
        got = nc.call_regions([F.region_from_arrays(r) for r in regs], ["S1"], default_options(), source_files=[(cli["vcf_gz"], idx)])
        assert got == want and nc.stats["n_source_lines"] == n_lines
        plain = nc.call_regions([F.region_from_arrays(r) for r in regs], ["S1"], default_options())       # (the files applied to one call)
        assert nc.stats["n_source_lines"] == 0 and plain != want
        idx.close()
    finally:
        nc.close()


def test_an_index_the_library_wrote_is_read_back_by_the_library():
    """compress -> index -> open -> set_source_files: the lines of the output, with no Python index code in the loop."""
    regs = [synth.config4_region_arrays(i, region_len=4000, n_samples=1, read_len=100) for i in range(3)]
    header = b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
    nc = F.NativeCaller(0, 2, 2)
    try:
        opts = default_options(rlen=100)
        opts.originalMaxHaplotypes = opts.maxHaplotypes
        text = nc.call_regions([F.region_from_arrays(r) for r in regs], ["S1"], opts).encode("ascii")
        lens = [int(x) for x in nc.region_text_lengths(3)]
        packed = bytes(nc.compress_text(header + text, [len(header)] + lens)[0])
        idx = nc.open_index(nc.index_bgzf(packed))
        records = [ln for ln in text.split(b"\n") if ln]
        span = lambda ln: (ln.split(b"\t")[0], int(ln.split(b"\t")[1]) - 1, int(ln.split(b"\t")[1]) - 1 + len(ln.split(b"\t")[3]))
        regions = [(r["chrom"].encode(), r["start"] + 1300 * k, r["start"] + 1300 * (k + 1) + 37) for r in regs for k in range(3)]
        nc.set_source_files([(packed, idx)], regions)
        got = nc.source_lines_set(len(regions))
        want = [b"".join(ln + b"\n" for ln in records if span(ln)[0] == c and span(ln)[2] > b and e > span(ln)[1]) for c, b, e in regions]
        assert got == want and sum(len(w) for w in want) > 1000
        assert [idx.tid(r["chrom"]) for r in regs] == sorted(set(idx.tid(r["chrom"]) for r in regs)) and idx.tid(b"nope") == -1
        idx.close()
    finally:
        nc.close()
