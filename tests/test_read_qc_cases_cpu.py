"""The inputs of tests/test_gpu_read_qc_fuzz.py (tests/read_qc_cases.py) on the CPU: the oracle's checkAndTrimRead against the CPU stand-in
device's (tests/fakedev/fake_device.c: a third statement of the rule, written apart from the oracle's and the device kernel's), and, on the
oracle alone, the conditions the inputs were written to reach -- every reason rejecting reads, every trimming rule changing reads that no other
rule touches, quality bytes of 128 and above in accepted reads, every listed length, stream size and CIGAR pair count -- without which the
comparisons on the device would hold without saying anything.  The figures asserted are conditions on the inputs, not measurements."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_qc_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def calls():
    return C.calls()


@pytest.fixture(scope="module")
def verdicts(calls, oracle):
    """Per call: its table and the oracle's (ok, reason, flags, qual) over it."""
    out = []
    for c in calls:
        tab = C.table_of(c["streams"])
        out.append((tab, C.oracle_table(oracle, tab, c["opt"])))
    return out


def reads_of(calls):
    return [r for c in calls for st in c["streams"] for r in st]


def changed_reads(tab, before, after):
    """Which reads of a table hold a byte that differs between two quality blobs."""
    n = len(tab["pos"])
    read_of_byte = np.repeat(np.arange(n), np.diff(tab["off"]))
    return np.bincount(read_of_byte[before != after], minlength=n) > 0


def test_the_oracle_equals_the_stand_in_device_on_every_stream(calls, verdicts):
    from tests.fakedev import fake_engine
    eng = fake_engine()
    n = 0
    for c, (tab, (ok, why, flags, qual)) in zip(calls, verdicts):
        streams = [[dict(r, qual=np.frombuffer(r["qual"], dtype=np.uint8)) for r in st] for st in c["streams"]]
        got = eng.read_qc(streams, *C.qc_args(c["opt"]))
        for s, (g_ok, g_flags, g_qual, g_why) in enumerate(got):
            a, z = int(tab["sbeg"][s]), int(tab["sbeg"][s + 1])
            assert np.array_equal(g_ok, ok[a:z]) and np.array_equal(g_why, why[a:z]) and np.array_equal(g_flags, flags[a:z]), (c["name"], s)
            mine = np.concatenate(g_qual) if g_qual else np.zeros(0, np.uint8)
            assert np.array_equal(mine, qual[int(tab["off"][a]):int(tab["off"][z])]), (c["name"], s)
            n += z - a
    assert n == len(reads_of(calls)) and n > 20000


def test_the_oracle_gives_the_same_from_dicts_and_from_arrays(calls, verdicts, oracle):
    """Oracle.check_and_trim (what the goldens pin) and check_and_trim_arrays (what the tables go through) on the fuzz streams."""
    n = 0
    for c, (tab, (ok, why, flags, qual)) in zip(calls, verdicts):
        if not c["name"].startswith("fuzz"):
            continue
        for s, st in enumerate(c["streams"]):
            a, z = int(tab["sbeg"][s]), int(tab["sbeg"][s + 1])
            d_ok, d_flags, d_qual, d_why = oracle.check_and_trim(st, c["opt"])
            assert np.array_equal(d_ok, ok[a:z]) and np.array_equal(d_why, why[a:z]) and np.array_equal(d_flags, flags[a:z])
            assert [x & 255 for q in d_qual for x in q] == qual[int(tab["off"][a]):int(tab["off"][z])].tolist()
            assert all(-128 <= x < 128 for q in d_qual for x in q)
            n += z - a
    assert n > 5000


def test_every_reason_rejects_and_enough_reads_are_accepted(verdicts):
    ok = np.concatenate([v[0] for _, v in verdicts])
    why = np.concatenate([v[1] for _, v in verdicts])
    assert set(why[ok == 0].tolist()) == set(range(8)) and (why[ok != 0] == -1).all()
    hist = np.bincount(why[ok == 0], minlength=8)
    for k, name in enumerate(C.REASONS):
        assert hist[k] >= 50, (name, hist.tolist())
    assert ok.mean() >= 0.30, ok.mean()
    # the two reasons that leave the QCFail flag alone, and the six that set it
    for tab, (ok_, why_, flags, _) in verdicts:
        sets = (ok_ == 0) & ~np.isin(why_, [2, 3])
        assert np.array_equal(flags, np.where(sets, tab["flags"] | 512, tab["flags"]))


def test_each_trimming_rule_changes_reads_that_no_other_rule_touches(calls, verdicts, oracle):
    """Rule by rule: the accepted reads that come out changed, and that come out unchanged once that rule is off.  The low-quality-end rule
    has no switch: it is off for a table whose bytes below 5 (1..4 and, as signed chars, 128..255) are 0 already -- which rejects no read
    that was accepted, so the accepted reads of the real table are looked at."""
    alone = dict(below5=0, flank=0, overlapping=0, adapter=0, soft=0)
    off = dict(flank=dict(trimReadFlank=0), overlapping=dict(trimOverlapping=0), adapter=dict(trimAdapter=0), soft=dict(trimSoftClipped=0))
    for c, (tab, (ok, why, flags, qual)) in zip(calls, verdicts):
        real = changed_reads(tab, tab["qual"], qual) & (ok != 0)
        for rule, kw in off.items():
            o2 = dict(c["opt"], **kw)
            ok2, _, _, q2 = C.oracle_table(oracle, tab, o2)
            assert np.array_equal(ok2, ok)                                             # no trimming option bears on a verdict
            alone[rule] += int((real & ~changed_reads(tab, tab["qual"], q2)).sum())
        flat = dict(tab, qual=np.where((tab["qual"] < 5) | (tab["qual"] >= 128), 0, tab["qual"]).astype(np.uint8))
        ok3, _, _, q3 = C.oracle_table(oracle, flat, c["opt"])
        assert (ok3[ok != 0] != 0).all()
        alone["below5"] += int((real & ~changed_reads(tab, flat["qual"], q3)).sum())
    for rule, n in alone.items():
        assert n >= 20, alone


def test_accepted_reads_hold_bytes_of_128_and_above_and_they_come_out_zero_or_unchanged(verdicts):
    n_reads = 0
    kept = trimmed = 0
    for tab, (ok, why, flags, qual) in verdicts:
        n = len(tab["pos"])
        read_of_byte = np.repeat(np.arange(n), np.diff(tab["off"]))
        high = (tab["qual"] >= 128) & (ok[read_of_byte] != 0)
        n_reads += len(np.unique(read_of_byte[high]))
        assert ((qual[high] == 0) | (qual[high] == tab["qual"][high])).all()
        kept += int((qual[high] != 0).sum()); trimmed += int((qual[high] == 0).sum())
        rejected = ok[read_of_byte] == 0
        assert np.array_equal(qual[rejected], tab["qual"][rejected])                   # a rejected read is not trimmed
    assert n_reads >= 200 and kept >= 200 and trimmed >= 200, (n_reads, kept, trimmed)


def test_the_inputs_hold_every_listed_shape(calls):
    reads = reads_of(calls)
    assert 20000 <= len(reads) <= 60000
    assert set(C.STREAM_SIZES) <= {len(st) for c in calls for st in c["streams"]}
    assert set(C.LENGTHS) <= {len(r["seq"]) for r in reads} and all(len(r["seq"]) == len(r["qual"]) for r in reads)
    assert set(C.PAIR_COUNTS) <= {len(r["cigar"]) for r in reads}
    assert {op for r in reads for op, ln in r["cigar"]} == set(range(9))
    assert all(C.consumed(r["cigar"]) <= len(r["seq"]) for r in reads)                  # past that the reference has no answer
    assert all(r["insertSize"] > -2 ** 31 for r in reads)
    # options: every listed value, all 16 settings of `enabled`
    for key, vals in (("minMapQual", C.MIN_MAP_QUALS), ("minBaseQual", C.MIN_BASE_QUALS), ("minGoodQualBases", C.MIN_GOOD_QUAL_BASES),
                      ("trimReadFlank", C.TRIM_READ_FLANKS), ("trimOverlapping", C.SWITCHES), ("trimAdapter", C.SWITCHES),
                      ("trimSoftClipped", C.SWITCHES)):
        assert set(vals) <= {c["opt"][key] for c in calls}, key
    assert len({tuple(c["opt"]["enabled"]) for c in calls}) == 16
    # qualities: below 5, the thresholds, the packed format's edge, both kinds of exception; mapq on both sides of every threshold
    for v in C.MIN_BASE_QUALS[1:]:
        q = set(b"".join(r["qual"] for c in calls if c["opt"]["minBaseQual"] == v for st in c["streams"] for r in st))
        assert {0, 1, 2, 3, 4, 5, v - 1, v, 63, 64} <= q and any(64 < x < 128 for x in q) and any(x >= 128 for x in q), v
    for v in C.MIN_MAP_QUALS:
        m = {r["mapq"] for c in calls if c["opt"]["minMapQual"] == v for st in c["streams"] for r in st}
        assert v in m and (v == 0 or v - 1 in m) and (v == 255 or any(x > v for x in m)), v
    assert sum(1 for r in reads if r["qual"] and max(r["qual"]) < 5) >= 20             # whole reads below 5
    # flags
    flags = {r["flag"] for r in reads}
    assert set(C.PAIR_FLAGS) | {0, 16} <= flags
    special = sum(C.SPECIAL_BITS)
    for b in C.SPECIAL_BITS:
        assert any(f & special == b for f in flags), b
    assert len({f & special for f in flags if bin(f & special).count("1") >= 2}) >= 8
    # insert sizes at the edges of the three rules that read them
    seen = set()
    for r in reads:
        L, i = len(r["seq"]), r["insertSize"]
        if L >= 3:
            for name, v in (("0", 0), ("1", 1), ("L-1", L - 1), ("L", L), ("L+1", L + 1), ("2L-1", 2 * L - 1), ("2L", 2 * L), ("2L+1", 2 * L + 1)):
                if abs(i) == v:
                    seen.add((name, i < 0))
        if abs(i) >= 100000:
            seen.add(("large", i < 0))
    assert len(seen) == 17, sorted(seen)                                                # 8 edges and "large" in both signs, but 0
    # CIGARs: a soft clip first, last, behind a hard clip, twice, and behind each operation that does not move the reference's cursor
    ops = [[op for op, ln in r["cigar"]] for r in reads]
    assert any(o[:1] == [C.S_] for o in ops) and any(len(o) > 1 and o[-1] == C.S_ for o in ops) and any(o[:2] == [C.H_, C.S_] for o in ops)
    assert any(o.count(C.S_) >= 2 for o in ops)
    for before in (C.EQ_, C.X_, C.SKIP_, C.P_, C.D_):
        assert any(o[k] == before and o[k + 1] == C.S_ for o in ops for k in range(len(o) - 1)), before


def test_duplicates_by_position_inside_a_stream_and_not_across_streams(calls, verdicts, oracle):
    by_pos = dict(paired=0, unpaired=0, other_mate=0, other_length=0)
    copies = 0
    for c, (tab, (ok, why, flags, qual)) in zip(calls, verdicts):
        k = 0
        for s, st in enumerate(c["streams"]):
            for i, r in enumerate(st):
                if i and r["pos"] == st[i - 1]["pos"]:
                    same_len = len(r["seq"]) == len(st[i - 1]["seq"])
                    if why[k + i] == 5 and not r["flag"] & 1024:
                        assert same_len
                        by_pos["paired" if r["flag"] & 1 else "unpaired"] += 1
                    elif ok[k + i] and same_len and c["opt"]["enabled"][3]:
                        assert r["flag"] & 1 and r["matePos"] != st[i - 1]["matePos"]
                        by_pos["other_mate"] += 1
                    elif ok[k + i] and not same_len and c["opt"]["enabled"][3]:
                        by_pos["other_length"] += 1
            if c["labels"][s].endswith("copies_last"):
                prev = c["streams"][s - 1]
                assert ok[k] == 1 and ok[k - 1] == 1 and C.clone(prev[-1]) == C.clone(st[0]) and c["opt"]["enabled"][3]
                merged = oracle.check_and_trim(prev + st, c["opt"])                    # in ONE stream the copy is a duplicate
                assert merged[0][len(prev)] == 0 and merged[3][len(prev)] == 5
                copies += 1
            k += len(st)
    assert copies >= 10 and all(v >= 20 for v in by_pos.values()), (copies, by_pos)


def test_verdict_patterns_and_stream_order(calls, verdicts):
    seen = set()
    for c, (tab, (ok, why, flags, qual)) in zip(calls, verdicts):
        for s, label in enumerate(c["labels"]):
            a, z = int(tab["sbeg"][s]), int(tab["sbeg"][s + 1])
            parts = label.split(":")
            if len(parts) >= 3 and parts[1] in C.PATTERNS:
                n, rejected = int(parts[0]), C.rejected_of(parts[1], int(parts[0]))
                assert z - a == n and set(np.nonzero(ok[a:z] == 0)[0].tolist()) == rejected, label
                assert (why[a:z][ok[a:z] == 0] == (6 if parts[2] == "mapq" else 5)).all()
                seen.add((n, parts[1]))
            descents = np.nonzero(np.diff(tab["pos"][a:z].astype(np.int64)) < 0)[0] + 1
            if label == "unsorted":
                assert len(descents) >= 1 and descents[0] % 512 != 0
            elif label == "descent@512":
                assert descents.tolist() == [512] and z - a > 512
            else:
                assert len(descents) == 0
        labels = c["labels"]
        if c["name"].startswith("patterns"):                                            # empty streams first, last and side by side
            assert labels[0] == labels[-1] == "empty" and any(labels[k] == labels[k + 1] == "empty" for k in range(len(labels) - 1))
    # all accepted, all rejected and alternating at every size; the single rejected read at every index that streams of 65, 513 and 1025 have
    assert seen == ({(n, p) for n in C.STREAM_SIZES[1:] for p in C.PATTERNS[:3]} | {(0, "all_accepted")} |
                    {(n, p) for n in (65, 513, 1025) for p in C.PATTERNS[3:] if C.rejected_of(p, n) is not None})
    assert {p for n, p in seen} == set(C.PATTERNS)


def test_the_long_stream(oracle):
    tab, opt = C.long_table(), C.long_options()
    n = len(tab["pos"])
    assert n == C.LONG_READS == 262144 + 700 and (np.diff(tab["pos"]) >= 0).all()
    lens = np.diff(tab["off"])
    assert lens.min() == 1 and lens.max() == 3 and (np.diff(tab["coff"]) <= 2).all()
    ok, why, flags, qual = C.oracle_table(oracle, tab, opt)
    assert 0.35 <= 1 - ok.mean() <= 0.45
    assert {5, 6} <= set(why[ok == 0].tolist())
    # irregular: the accepted counts of the 512-read tiles and of the 64-read waves take many values, and the reads past the masks kept in
    # LDS are of both kinds
    tiles = np.add.reduceat(ok, np.arange(0, n, 512))
    assert len(set(tiles.tolist())) > 50 and 0 < ok[262144:].sum() < 700
    assert (qual != tab["qual"]).sum() > 1000
