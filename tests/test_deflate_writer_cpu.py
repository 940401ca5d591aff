"""CPU tests of the test suite's own deflate writer (tests/deflate_writer.py) and of the cases built with it (tests/bgzf_cases.py:
foreign_blocks, foreign_fuzz, walk_seam_cases) -- against zlib alone.  Nothing here runs the code under test: these tests say that the
streams are what they claim to be (valid where zlib inflates them to the payload, refused where zlib refuses them) and that they REACH
what they were written to reach, read from the writer's own records of what it emitted, from zlib's error messages and from the walk
rule's offsets.  tests/test_bgzf_cpu.py feeds the same cases to the host build, tests/test_gpu_bgzf_foreign.py to the device."""
import struct
import zlib

import numpy as np
import pytest

from tests import bgzf_cases as K
from tests import deflate_writer as D


def _cdata(block):
    xlen = struct.unpack_from("<H", block, 10)[0]
    return block[12 + xlen:len(block) - 8]


def test_the_writers_parts_by_hand():
    # the fixed code's 'A' and the stored block of "ACGT", as tests/bgzf_cases.py and the BGZF writer's test state them
    assert D.canonical(D.FIXED_LIT)[0x41] == K.FIXED_A and D.canonical(D.FIXED_LIT)[256] == "0000000" and D.canonical(D.FIXED_DIST)[1] == "00001"
    assert D.DeflateWriter().stored(b"ACGT", final=True).finish().hex() == "01" "0400" "fbff" "41434754"
    # RFC 1951's own example (3.2.2): lengths 3 3 3 3 3 2 4 4 -> codes 010 011 100 101 110 00 1110 1111
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == dict(enumerate(["010", "011", "100", "101", "110", "00", "1110", "1111"]))
    assert D.length_symbol(3) == (257, 0) and D.length_symbol(258) == (285, 0) and D.length_symbol(257) == (284, 30) and D.length_symbol(11) == (265, 0)
    assert D.dist_symbol(1) == (0, 0) and D.dist_symbol(32768) == (29, 8191) and D.dist_symbol(5) == (4, 0) and D.dist_symbol(24576) == (28, 8191)
    lad = D.ladder_lengths(list(range(16)), 20)
    assert lad[:16] == list(range(1, 16)) + [15] and D.kraft(lad) == 1 << 15
    assert sorted(D.ladder_lengths([0, [1, 2, 3, 4], 5], 6)) == [1, 2, 4, 4, 4, 4]
    for n in (2, 3, 5, 8, 19, 30, 286):
        assert D.kraft(D.flat_lengths(range(n), 288)) == 1 << 15
    rng = np.random.default_rng(1)
    for n, maxlen in ((2, 7), (19, 7), (30, 15), (286, 15), (17, 15)):
        for deep in (0.0, 0.5, 1.0):
            lens = D.random_lengths(rng, list(range(n)), 288, maxlen, deep)
            assert D.kraft(lens) == 1 << 15 and max(lens) <= maxlen and sum(1 for l in lens if l) == n
    assert max(D.random_lengths(rng, list(range(17)), 20, 15, 1.0)) == 15
    for kind, lens in (("lit", [1, 1, 1]), ("lit", [2, 2]), ("dist", [2]), ("lit", [0, 0]), ("cl", [1]), ("cl", [0])):
        with pytest.raises(AssertionError):
            D.check_code(lens, kind)
    for kind, lens in (("lit", [1]), ("dist", [0, 1]), ("dist", [0, 0]), ("cl", [1, 1]), ("lit", [1, 2, 2])):
        D.check_code(lens, kind)
    seq = [3] * 9 + [0] * 150 + [5, 5, 5, 0, 0, 7] + [0] * 12
    for ops in (D.rle_none(seq), D.rle_greedy(seq), D.rle_random(seq, rng), D.rle_random(seq, rng)):
        assert D.rle_expand(ops) == seq
    assert D.rle_greedy(seq) == [(3, 1), (16, 6), (3, 1), (3, 1), (18, 138), (18, 12), (5, 1), (5, 1), (5, 1), (0, 1), (0, 1), (7, 1), (18, 12)]
    # the matcher gives the data back, keeps its limits and stops at the cuts
    data = K._text(5, 3000) + bytes(600) + K._text(6, 500)
    for max_dist, min_len, cuts in ((32768, 3, ()), (1, 3, ()), (100, 8, (7, 1000, 3001)), (5, 30, (3600,))):
        toks = D.match_tokens(data, max_dist, min_len, cuts=cuts)
        assert bytes(D.replay(toks)) == data
        assert all(min_len <= t[0] <= 258 and 1 <= t[1] <= max_dist for t in toks if not isinstance(t, int))
        parts = D.split_tokens(toks, cuts)
        edges = [0] + sorted(cuts) + [len(data)]
        assert len(parts) == len(edges) - 1 and [sum(D.token_span(t)[0] for t in p) for p in parts] == [b - a for a, b in zip(edges, edges[1:])]
    assert any(not isinstance(t, int) and t[0] > t[1] for t in D.match_tokens(data))                      # (an overlapping match)
    # a writer that is asked for an invalid stream without check=False refuses
    with pytest.raises(AssertionError):
        D.DeflateWriter().dynamic([97], [0] * 97 + [1], [0])                                                # no code for 256
    with pytest.raises(AssertionError):
        D.DeflateWriter().dynamic([], D.single_lengths(256, 288), [0], rle=[(18, 138), (18, 121)])            # a run past HLIT + HDIST


def test_every_valid_stream_inflates_to_its_payload_with_zlib_alone():
    blocks = K.foreign_blocks()
    fuzz, _ = K.foreign_fuzz()
    assert len(fuzz) == 400 and len(blocks) >= 250
    n_valid = 0
    for name, payload, block, *_ in blocks + fuzz:
        want = K.reference_verdict(block)
        # a hand-written None is only a claim: zlib decides, and the claim has to agree; a stream the writer calls valid and zlib refuses
        # is a bug of the writer
        assert (payload is None) == (want is None), (name, K.zlib_message(block))
        assert len(block) <= 65536, name
        if payload is None:
            continue
        d = zlib.decompressobj(-15)
        assert d.decompress(_cdata(block)) == payload and d.eof and want == payload, name
        n_valid += 1
    assert n_valid >= 630
    sizes = [len(p) for _, p, _, _ in fuzz]
    assert min(sizes) == 0 and max(sizes) == 65536 and {n.split(" of ")[1].split(" in ")[0] for n, *_ in fuzz} == {"records", "four letters", "random"}
    assert max(len(p) for _, p, _ in blocks if p is not None) == 65536
    # what does not fit a BGZF block: 65536 bytes as stored 65535 + stored 1 (BSIZE allows 65510 bytes of deflate data) -- the writer and zlib
    big = np.random.default_rng(4).integers(0, 256, size=65536, dtype=np.uint8).tobytes()
    d = zlib.decompressobj(-15)
    assert d.decompress(D.DeflateWriter().stored(big[:65535]).stored(big[65535:], final=True).finish()) == big and d.eof
    # the fuzz is seeded: the same streams again
    again, _ = K.foreign_fuzz(n=12)
    assert [a[2:] for a in again] == [f[2:] for f in fuzz[:12]]


def test_the_cases_reach_what_they_were_written_for():
    """From the writer's records and zlib's messages, never from the code under test."""
    blocks, rec = K.foreign_blocks(), D.Records()
    fuzz, fuzz_rec = K.foreign_fuzz()
    valid = [b for b in blocks if b[1] is not None]
    names = {n for n, _, _ in blocks}
    rec.merge(K.foreign_records()).merge(fuzz_rec)
    full = set(range(1, 16))
    assert rec.lit_lens >= full and rec.dist_lens >= full and 7 in rec.cl_lens
    # ... and by the named cases alone, the fuzz aside
    named = K.foreign_records()
    assert named.lit_lens >= full and named.dist_lens >= full and 7 in named.cl_lens
    both = {"zero", "one"}
    assert sorted(named.len_syms) == list(range(257, 286)) and all(v == both for v in named.len_syms.values())
    assert sorted(named.dist_syms) == list(range(30)) and all(v == both for v in named.dist_syms.values())
    assert set(named.stored_phases) == set(range(8)) and set(fuzz_rec.stored_phases) == set(range(8))
    assert named.rle_modes == fuzz_rec.rle_modes == {"none", "greedy", "explicit"}
    assert named.cross16 >= 1 and named.cross18 >= 1 and fuzz_rec.cross18 >= 1
    assert set(named.blocks) == set(fuzz_rec.blocks) == {"stored", "fixed", "dynamic"}
    # the ladders are whole
    for dist in K.OVERLAP_DISTS:
        for ln in K.OVERLAP_LENS:
            assert "overlap dist %d len %d" % (dist, ln) in names
    assert len(K.OVERLAP_DISTS) * len(K.OVERLAP_LENS) == 126 and all("chain behind %d literals" % s in names for s in range(67))
    # the chain's links: commands 3 + shift .. 10 + shift of the block -- every link falls on each of the slots 62..65 for some shift
    assert all(any(3 + s + link == slot for s in range(67)) for link in range(8) for slot in (62, 63, 64, 65))
    assert sum(1 for _, p, _ in valid if len(p) == 65536) >= 2 and any(len(p) == 0 for _, p, _ in valid)
    # zlib's refusals, over the refused named cases and the flipped fuzz streams
    refused = [b for n, p, b in blocks if p is None] + [f for _, _, _, f in fuzz]
    said = {K.zlib_message(b) for b in refused}
    for msg in ("invalid block type", "invalid stored block lengths", "too many length or distance symbols", "invalid code lengths set", "invalid bit length repeat",
                "invalid code -- missing end-of-block", "invalid literal/lengths set", "invalid distances set", "invalid literal/length code",
                "invalid distance code", "invalid distance too far back"):
        assert any(s.endswith(msg) for s in said), msg
    verdicts = [K.reference_verdict(f) for _, _, _, f in fuzz]
    harmless = sum(1 for v, (_, p, _, _) in zip(verdicts, fuzz) if v is not None)
    print("flipped fuzz streams: %d refused, %d still inflate to the payload" % (400 - harmless, harmless))
    assert 300 <= 400 - harmless < 400                                       # (a flip of BFINAL in front of trailing bytes, of a padding bit, of an unused length)


def test_the_walk_ladder_puts_a_record_at_every_distance_from_a_windows_end():
    cases, probes = K.walk_seam_cases()
    assert K.FIND_WINDOW == 16384 and K.window_base(16387) == 16384
    seen, straddles, ends = set(), set(), []
    for i, (name, data, first, stop, tid, beg, end) in enumerate(cases):
        assert 32000 <= len(data) <= 70000, name
        rc, kept, walked, ended = K.rule_walk(data, first, stop, tid, beg, end)
        assert rc == 0 and walked == len(kept) > 100 and not ended, name                       # every record is kept: the offsets are all the records' starts
        starts = [k - 4 for k in kept]
        assert starts[0] == first
        needs = [K.record_need(data[s:s + 20]) for s in starts]
        bases = K.window_bases(starts, needs, len(data))
        assert len(bases) >= 2, name
        if "stream ends" in name:
            ends.append(len(data) - bases[1] - K.FIND_WINDOW)
        if i not in probes:
            continue
        d, probe = probes[i]
        assert len(bases) >= 3, name
        assert len(data) % 4 == 0                                                                # (side by side in one call the bases stay)
        w_end = bases[1] + K.FIND_WINDOW                                                         # the second window: its base is where the first one broke
        assert bases[1] == K.window_base(starts[[s + n <= K.window_base(first) + K.FIND_WINDOW for s, n in zip(starts, needs)].index(False)])
        assert probe in starts and w_end - probe == d, name
        seen.add(d)
        straddles.add((d, probe + needs[starts.index(probe)] - w_end))
    assert seen == set(range(45))
    # the last CIGAR word's end against the window's end, for every d that leaves room for a name
    for d in range(45):
        for delta in (-4, -1, 0, 1, 4):
            assert (d - 36 + delta < 1) or (d, delta) in straddles, (d, delta)
    assert {first for _, _, first, *_ in cases} == {0, 1, 2, 3}
    assert ends == list(range(41))
    assert sum("longer than a window" in c[0] for c in cases) == 2
