"""plat_stage_b_batch on seeded regions past the committed goldens (tests/stage_b_cases.py; tests/test_stage_b_cases_cpu.py proves on the
mirror alone what those inputs reach) against tests/stage_b_reference.py, the mirror chain.  All integers and bytes: every comparison is
exact.  R.compare() is run on EVERY call of this file: hdr (status AND reason code), every variant / window / batch array by content, and the
sentinel in every element behind what the counts say was written.  Each test is one or a few launches."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_b_cases as C  # noqa: E402
import stage_b_reference as R  # noqa: E402
from test_gpu_stage_b_kernels import _StopOnDeviceError, eng  # noqa: E402,F401  (a HIP error ends the session: nothing more is started)
from platypus_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

TALLY = {}


def run(eng, regions, o, cp, cap_per_scan=None, name=None):
    """One plat_stage_b_batch call on the generator's candidates, compared with the mirror in full.  -> (arrays, expectation, packed arguments)"""
    a = R.pack(regions, cap_per_scan)
    out = eng.stage_b(a["regions"], a["tables"], o, cand=a["cand"], cand_n=a["cand_n"], read_seq=a["read_seq"], cap_per_scan=a["cap_per_scan"], **cp)
    exp = R.expected(regions, o, cp, a["cap_per_scan"])
    R.compare(out, exp, regions, cp, Engine.sentinel_of)
    if name:
        t = TALLY.setdefault(name, dict(calls=0, regions=0, flagged=0, variants=0, windows=0, batch_windows=0, haplotypes=0))
        t["calls"] += 1
        for k, v in R.counts(exp).items():
            t[k] += v
        print("[stage-b fuzz] %s: %s" % (name, json.dumps(t)))
    return out, exp, a


def batch_windows(out, n_regions):
    return [(g, k) for g in range(n_regions) if out["hdr"][g, 0] == 0 for k in range(out["hdr"][g, 2]) if out["win_flags"][g, k] in (0, R.SBW_DUPLICATE)]


def check_sums(out, regions, a):
    """The totals and every prefix array against sums recomputed from the per-window outputs."""
    tot = out["totals"].tolist()
    nw, nh, nr = tot[:3]
    assert tot[10] == 0
    wins = batch_windows(out, len(regions))
    assert [int(out["win_batch"][g, k]) for g, k in wins] == list(range(nw))
    n_haps = [int(out["win_n_haps"][g, k]) for g, k in wins]
    n_reads = [int(sum(out["win_ptrs"][g, k, 2 * t + 1] - out["win_ptrs"][g, k, 2 * t] for t in range(3))) for g, k in wins]
    cum = lambda xs: np.concatenate([[0], np.cumsum(xs, dtype=np.int64)]).tolist()
    assert out["b_hap_begin"][:nw + 1].tolist() == cum(n_haps) and out["b_read_begin"][:nw + 1].tolist() == cum(n_reads) == out["b_seg_begin"][:nw + 1].tolist()
    assert out["b_pair_off"][:nw + 1].tolist() == cum([h * r for h, r in zip(n_haps, n_reads)])
    assert out["b_gl_off"][:nw + 1].tolist() == cum([h * (h + 1) // 2 for h in n_haps])
    assert tot[:5] == [nw, sum(n_haps), sum(n_reads), sum(h * r for h, r in zip(n_haps, n_reads)), sum(h * (h + 1) // 2 for h in n_haps)]
    lens = np.diff(out["b_hap_off"][:nh + 1])
    assert tot[5] == lens.sum() == out["b_hap_off"][nh] and tot[7] == (lens.max() if nh else 0) and tot[8] == max(n_reads, default=0) and tot[9] == max(n_haps, default=0)
    read_len = np.diff(a["tables"]["read_off"])
    assert out["b_read_off"][:nr + 1].tolist() == cum(read_len[out["b_read_src"][:nr]]) and tot[6] == out["b_read_off"][nr]
    for (g, k), bw in zip(wins, range(nw)):
        r0 = int(out["b_read_begin"][bw])
        want = [(a["tables"]["tab_begin"][3 * g + t] + i, t) for t in range(3) for i in range(out["win_ptrs"][g, k, 2 * t], out["win_ptrs"][g, k, 2 * t + 1])]
        assert list(zip(out["b_read_src"][r0:r0 + len(want)].tolist(), out["b_read_kind"][r0:r0 + len(want)].tolist())) == want
        assert out["b_n_good"][bw] == out["win_ptrs"][g, k, 1] - out["win_ptrs"][g, k, 0]
        assert (int(out["b_start"][bw]), int(out["b_end"][bw]), int(out["b_flank"][bw])) == (
            max(int(out["win_start"][g, k]), 0), min(int(out["win_end"][g, k]), regions[g]["contig_len"] - 1), min(2 * regions[g]["rlen"], 500))
    return nw, nh, nr


# ---- the corpus, option set by option set ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(13))
def test_the_corpus_equals_the_mirror(eng, k):
    calls = C.corpus()
    assert len(calls) == 13
    c = calls[k]
    out, exp, a = run(eng, c["regions"], c["o"], c["cp"], name=c["name"])
    if not exp["batch"]["totals"][10]:
        check_sums(out, c["regions"], a)


# ---- the size ladder -------------------------------------------------------------------------------------------------------------------------------

def test_the_size_ladder(eng):
    lad = C.ladder()
    c = lad["candidates"]                                                         # 63 / 64 / 65 and 1 000 .. 1 024 candidates: the strides of the sorts
    out, exp, a = run(eng, c["regions"], c["o"], c["cp"], name=c["name"])
    n = a["cand_n"][:, 0].tolist()
    assert n[:7] == [0, 1, 2, 63, 64, 65, 200] and 1000 <= n[7] <= 1024 and (out["hdr"][:, 0] == 0).all()
    assert out["hdr"][7, 1] > 500 and out["hdr"][3:6, 1].min() > 30
    c = lad["indels"]                                                             # 15 / 16 / 17 / 33 indels: one, two and three trips of the 16 waves
    out, exp, a = run(eng, c["regions"], c["o"], c["cp"], name=c["name"])
    assert [sum(C.pure_indel(x) and x[0] >= 100 for x in reg["cands"]) for reg in c["regions"]] == [0, 1, 15, 16, 17, 33] and (out["hdr"][:, 0] == 0).all()
    kept = [sum(int(out["var_nrem"][g, i]) != int(out["var_nadd"][g, i]) for i in range(out["hdr"][g, 1])) for g in range(6)]
    assert kept[0] == 0 and kept[1] <= 1 and 10 <= kept[2] <= 15 and kept[5] > 20
    c = lad["runs"]                                                               # 1 / 2 / 3 / 48 / 49 candidates of one key after normalisation
    out, exp, a = run(eng, c["regions"], c["o"], c["cp"], name=c["name"])
    assert out["hdr"][:, 0].tolist() == [0, 0, 0, 0, 1] and out["hdr"][4, 5] == 2
    assert out["hdr"][:4, 1].tolist() == [1, 1, 1, 1] and out["var_support"][3, 0] == sum(2 + i % 3 for i in range(48))
    c = lad["windows"]                                                            # 255 / 256 / 257 / 370 windows: the strides of k_sb_windows and k_sb_prefix
    out, exp, a = run(eng, c["regions"], c["o"], c["cp"], name=c["name"])
    assert out["hdr"][:, 2].tolist() == [255, 256, 257, 370, 1, 0] and (out["hdr"][:, 0] == 0).all()
    check_sums(out, c["regions"], a)


# ---- regions per call ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_regions_per_call(eng, n):
    """k_sb_scan strides by 64: flagged and unflagged, loaded and empty regions as the draw brings them."""
    regions = C.draw(n, 500 + n)
    if n == 1:
        regions = [C.corpus()[3]["regions"][-1]]                                  # (ten windows of 1..5 variants)
    out, exp, a = run(eng, regions, R.options(maxHaplotypes=33), R.caps(**C.BIG), name="regions per call")
    nw, nh, nr = check_sums(out, regions, a)
    assert nw >= 5
    if n >= 63:
        flagged = int((out["hdr"][:, 0] != 0).sum())
        assert 0 < flagged < n // 2 and nw > n and any(not reg["cands"] for reg in regions)


# ---- capacities ------------------------------------------------------------------------------------------------------------------------------------

def test_every_capacity_exactly_full_and_one_under(eng):
    c = C.corpus()[9]
    out, exp, a = run(eng, c["regions"], c["o"], c["cp"], name="capacities")
    assert (out["hdr"][:, 0] == 0).all()
    tot = out["totals"].tolist()
    full = dict(cap_vars=int(out["hdr"][:, 1].max()), cap_windows=int(out["hdr"][:, 2].max()), cap_added=int(out["hdr"][:, 4].max()), cap_batch_windows=tot[0],
                cap_batch_haps=tot[1], cap_batch_reads=tot[2], cap_hap_bytes=tot[5])
    assert min(full.values()) > 1
    out2, exp2, _ = run(eng, c["regions"], c["o"], R.caps(**full), name="capacities")
    assert (out2["hdr"][:, 0] == 0).all() and out2["totals"].tolist() == tot and (out2["b_hap_seq"] == out["b_hap_seq"][:tot[5]]).all()
    for k in full:
        out3, exp3, _ = run(eng, c["regions"], c["o"], R.caps(**dict(full, **{k: full[k] - 1})), name="capacities")
        if k in ("cap_vars", "cap_windows", "cap_added"):
            col = dict(cap_vars=1, cap_windows=2, cap_added=4)[k]
            want = [int(x == full[k]) for x in out["hdr"][:, col].tolist()]
            assert out3["hdr"][:, 0].tolist() == want and sum(want) >= 1 and all(out3["hdr"][g, 5] == 6 for g, w in enumerate(want) if w)
        else:
            assert out3["totals"][10] != 0 and out3["totals"][:10].tolist() == tot[:10] and (out3["hdr"][:, 0] == 0).all()


# ---- order independence ----------------------------------------------------------------------------------------------------------------------------

def test_the_order_of_regions_and_a_second_call_change_nothing(eng):
    c = C.corpus()[5]
    regions = c["regions"]
    out, exp, a = run(eng, regions, c["o"], c["cp"], name="order")
    again, _, _ = run(eng, regions, c["o"], c["cp"], name="order")
    for k in out:
        if k not in ("var_add_off", "added"):
            assert (out[k] == again[k]).all(), k
    perm = np.random.default_rng(77).permutation(len(regions)).tolist()
    other, exp2, _ = run(eng, [regions[i] for i in perm], c["o"], c["cp"], name="order")
    for j, i in enumerate(perm):                                                  # region i of the first call is region j of the permuted one
        assert out["hdr"][i].tolist() == other["hdr"][j].tolist()
        if out["hdr"][i, 0]:
            continue
        nv, nw = int(out["hdr"][i, 1]), int(out["hdr"][i, 2])
        for k in ("var_pos", "var_nrem", "var_nadd", "var_support", "var_bam_min", "var_bam_max"):
            assert (out[k][i, :nv] == other[k][j, :nv]).all(), (i, k)
        for k in ("win_start", "win_end", "win_var_first", "win_var_n", "win_flags", "win_n_haps", "win_ptrs"):
            assert (out[k][i, :nw] == other[k][j, :nw]).all(), (i, k)
        for w in range(nw):
            b0, b1 = int(out["win_batch"][i, w]), int(other["win_batch"][j, w])
            assert (b0 < 0) == (b1 < 0)
            if b0 >= 0:
                h0, h1 = int(out["b_hap_begin"][b0]), int(other["b_hap_begin"][b1])
                nh = int(out["win_n_haps"][i, w])
                x = out["b_hap_seq"][out["b_hap_off"][h0]:out["b_hap_off"][h0 + nh]]
                y = other["b_hap_seq"][other["b_hap_off"][h1]:other["b_hap_off"][h1 + nh]]
                if out["win_flags"][i, w] == 0:
                    assert (x == y).all() and (out["b_hap_mask"][h0:h0 + nh] == other["b_hap_mask"][h1:h1 + nh]).all(), (i, w)


# ---- the dictionary replay from real scans -----------------------------------------------------------------------------------------------------------

def test_the_replayed_dictionaries_on_both_sides_of_every_rebuild(eng):
    """Scans of 5 .. 2 000 distinct records, of which four pass the support filter: the first dictionary is rebuilt at 6, 22, 86, 342 and
    1 366 keys, and the order of the two alleles of a site is what it yields."""
    from platypus_amd.vcfrecords import _py2_string_hash
    mpr = 32
    scans = [C.replay_scan(300 + k, n) for k, n in enumerate(C.REPLAY_TARGETS)]
    eng.candidates(scans, max_per_read=mpr, retry=False, keep_device=True)
    lc = eng.last_candidates
    assert (lc["status"] == 0).all()
    blob = lc["read_seq"].tobytes()
    begin = np.concatenate([[0], np.cumsum([len(s["reads"]) for s in scans])]).tolist()
    ends = [r["end"] for s in scans for r in s["reads"]]
    cap = 16
    cand, n = eng.candidates_merge(begin, ends, [150] * len(scans), 0.05, cap)
    assert (n[:, 1] == 0).all() and n[:, 0].tolist() == [4] * len(scans), n.tolist()
    regions, records = [], []
    for g, s in enumerate(scans):
        cands, distinct = C.scan_records(lc["rec"], lc["count"], blob, s, begin[g], mpr, cand[g, :n[g, 0]])
        assert sum(d[3] is not None for d in distinct) == len(cands) == 4
        regions.append(R.region(s["ref"], cands, rlen=150, start=300, end=2700, reads=[(r["pos"], r["end"], len(r["seq"])) for r in s["reads"]]))
        records.append(distinct)
    sizes = [len(d) for d in records]
    print("[stage-b fuzz] replay: distinct records per scan %s" % sizes)
    for lo, t, hi in ((0, 6, 22), (6, 22, 86), (22, 86, 342), (86, 342, 1366), (342, 1366, R.SB_CAP * 8)):
        assert any(lo <= x < t for x in sizes) and any(t <= x < hi for x in sizes), (t, sizes)
    assert sizes == list(C.REPLAY_TARGETS)
    a = R.pack(regions)
    h = _py2_string_hash("20")
    gd = [dict(start=300, end=2700, rlen=150, name_hash=h - (1 << 64) if h >= 1 << 63 else h) for _ in scans]
    o, cp = R.options(), R.caps()
    out = eng.stage_b(gd, a["tables"], o, with_records=True, **cp)
    exp = R.expected(regions, o, cp, cap, exact_records=records)
    assert all(e["replay"] == 1 and e["status"] == 0 and len(e["variants"]) == 4 for e in exp["regions"])
    R.compare(out, exp, regions, cp, Engine.sentinel_of)
    assert (out["hdr"][:, 6] == 1).all() and (out["hdr"][:, 1] == 4).all()
    orders = {tuple(out["added"][g, out["var_add_off"][g, i]] for i in range(4)) for g in range(len(scans))}
    print("[stage-b fuzz] replay: %s, %d different allele orders" % (json.dumps(R.counts(exp)), len(orders)))
    # the same candidates without the scan's records: the order is the dictionary's, the regions the caller's
    out = eng.stage_b(gd, a["tables"], o, with_records=False, **cp)
    exp = R.expected(regions, o, cp, cap)
    assert all(e["reason"] == 2 for e in exp["regions"])
    R.compare(out, exp, regions, cp, Engine.sentinel_of)
    assert out["hdr"][:, [0, 5]].tolist() == [[1, 2]] * len(scans)


def test_a_scan_beyond_the_dictionary_capacity_is_the_callers(eng):
    """More than SB_DICT_CAP (5 400) distinct records in one scan: the dictionary is not replayed, the region comes back with reason 2."""
    from platypus_amd.vcfrecords import _py2_string_hash
    mpr = 32
    scan = C.replay_scan(399, 5500, step=2)
    eng.candidates([scan], max_per_read=mpr, retry=False, keep_device=True)
    lc = eng.last_candidates
    assert (lc["status"] == 0).all()
    n_reads = len(scan["reads"])
    cand, n = eng.candidates_merge([0, n_reads], [r["end"] for r in scan["reads"]], [150], 0.05, 16)
    assert n.tolist() == [[4, 0]], n.tolist()
    cands, distinct = C.scan_records(lc["rec"], lc["count"], lc["read_seq"].tobytes(), scan, 0, mpr, cand[0, :4])
    print("[stage-b fuzz] replay: %d distinct records in one scan" % len(distinct))
    assert len(distinct) == 5500 > R.SB_DICT_CAP
    reg = R.region(scan["ref"], cands, rlen=150, start=300, end=2700, reads=[(r["pos"], r["end"], len(r["seq"])) for r in scan["reads"]])
    a = R.pack([reg])
    h = _py2_string_hash("20")
    gd = [dict(start=300, end=2700, rlen=150, name_hash=h - (1 << 64) if h >= 1 << 63 else h)]
    o, cp = R.options(), R.caps(cap_batch_reads=4096)
    out = eng.stage_b(gd, a["tables"], o, with_records=True, **cp)
    exp = R.expected([reg], o, cp, 16, exact_records=[distinct])
    assert exp["regions"][0]["reason"] == 2
    R.compare(out, exp, [reg], cp, Engine.sentinel_of)
    assert out["hdr"][0, [0, 5]].tolist() == [1, 2]
