"""GPU tests of the BGZF front end: plat_bgzf_inflate_batch against Python's zlib on the grid, the corrupt corpus and the record-walk cases
the host build of the same code has passed (tests/test_bgzf_cpu.py, tests/bgzf_cases.py), and plat_call_bgzf_regions against
plat_call_bam_regions on the same records (tests/test_gpu_bam_records.py pins that path to the fetched path and through it to the
reference's 245 lines).  The refusals here exercise error returns on inputs the sanitized host build refused first; none provokes a fault.

Expected record lists come from bgzf_cases.rule_walk, the rule restated, never from the code under test."""
import gzip
import json
import os
import struct
import zlib

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options
from tests import bgzf_cases as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _place(blocks, gaps):
    """Blocks in one blob with gap bytes in front of each: (blob, offsets)."""
    parts, off, at = [], [], 0
    for b, g in zip(blocks, gaps):
        parts.append(b"\xa5" * g)
        at += g
        off.append(at)
        parts.append(b)
        at += len(b)
    return b"".join(parts), np.array(off, dtype=np.int64)


def test_inflate_grid_on_the_device():
    eng = H.get_engine()
    grid = K.inflate_grid()
    blocks = [b for _, _, b in grid]
    payloads = [p for _, p, _ in grid]
    # BC behind another subfield, and EOF blocks in the middle
    blocks[5:5] = [synth.bgzf_block(b"behind another subfield", extra_subfields=b"XY\x03\x00abc" + b"BC\x01\x00z"), synth.BGZF_EOF]
    payloads[5:5] = [b"behind another subfield", b""]
    blocks[40:40] = [synth.BGZF_EOF, synth.BGZF_EOF]
    payloads[40:40] = [b"", b""]
    gaps = [(3, 1, 2, 5, 0, 7)[i % 6] for i in range(len(blocks))]
    blob, off = _place(blocks, gaps)
    assert {int(o) & 3 for o in off} == {0, 1, 2, 3}                       # blocks at all four byte alignments
    got = eng.bgzf_inflate(blob, off)
    total = sum(len(p) for p in payloads)
    assert list(got["status"]) == [0, -1, total, 0] and got["guard_intact"]
    assert list(got["out_off"]) == [0] + list(np.cumsum([len(p) for p in payloads]))
    data = got["data"].tobytes()
    for i, p in enumerate(payloads):
        a = int(got["out_off"][i])
        assert data[a:a + len(p)] == p, i
    assert zlib.crc32(data) == zlib.crc32(b"".join(payloads))
    # the same blocks with limits: each block's own end
    lim = off + np.array([len(b) for b in blocks])
    got = eng.bgzf_inflate(blob, off, blk_limit=lim)
    assert list(got["status"]) == [0, -1, total, 0] and got["data"].tobytes() == data
    # an empty batch
    got = eng.bgzf_inflate(b"", np.zeros(0, np.int64))
    assert list(got["status"]) == [0, -1, 0, 0] and got["guard_intact"] and list(got["out_off"]) == [0]


def test_70000_blocks_in_one_call():
    eng = H.get_engine()
    rng = np.random.default_rng(70)
    recs = K.synthetic_record_bytes(40000)
    kinds = [(recs[k * 300:k * 300 + 100 + 3 * k], (1, 6, 9)[k % 3], (0, zlib.Z_FIXED, 0, zlib.Z_RLE)[k % 4]) for k in range(60)]
    kinds += [(rng.integers(0, 256, size=50 + k, dtype=np.uint8).tobytes(), 6, 0) for k in range(10)] + [(b"", 6, 0)]
    made = [(p, synth.bgzf_block(p, lv, st)) for p, lv, st in kinds]
    pick = rng.integers(0, len(made), size=70000)
    blob, off = _place([made[k][1] for k in pick], [int(g) for g in rng.integers(0, 4, size=70000)])
    want = b"".join(made[k][0] for k in pick)
    got = eng.bgzf_inflate(blob, off)
    assert list(got["status"]) == [0, -1, len(want), 0] and got["guard_intact"]
    assert got["data"].tobytes() == want
    assert list(np.diff(got["out_off"])) == [len(made[k][0]) for k in pick]


def test_refused_blocks_name_the_lowest_and_leave_the_others_inflated():
    eng = H.get_engine()
    good_payloads = [b"first block " * 50, K.synthetic_record_bytes(9000), bytes(5000), b"last block " * 70]
    good = [synth.bgzf_block(p, lv) for p, lv in zip(good_payloads, (6, 1, 9, 0))]
    bad = K.corrupt_blocks()

    def check_others(got, payloads, skip):
        data = got["data"].tobytes()
        for i, p in enumerate(payloads):
            if i not in skip:
                a = int(got["out_off"][i])
                assert data[a:a + len(p)] == p, i

    for why, block in bad.items():
        for at in (0, 2, 4):
            blocks = good[:at] + [block] + good[at:]
            payloads = good_payloads[:at] + [None] + good_payloads[at:]
            blob, off = _place(blocks, [1] * len(blocks))
            lim = off + np.array([len(b) for b in blocks])                   # (a block whose BSIZE says more than its bytes must not read its neighbour)
            got = eng.bgzf_inflate(blob, off, blk_limit=lim, cap_bytes=sum(len(p) for p in good_payloads) + 70000, check=False)
            assert list(got["status"][:2]) == [-9, at], (why, at, got["status"])
            assert got["guard_intact"], why
            check_others(got, payloads, {at})
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                eng.bgzf_inflate(blob, off, blk_limit=lim, cap_bytes=sum(len(p) for p in good_payloads) + 70000)
            assert e.value.code == -9 and ("block %d" % at) in str(e.value)
    blob, off = _place(good, [2] * 4)
    total = sum(len(p) for p in good_payloads)
    ok = eng.bgzf_inflate(blob, off)                                          # the context is usable
    assert list(ok["status"]) == [0, -1, total, 0] and ok["data"].tobytes() == b"".join(good_payloads)
    # an offset below 0 or outside the blob, a block past its limit, a blob that ends inside the last block's trailer; two bad blocks: the lowest
    for o in (-1, len(blob) - 20, len(blob) + 100):
        got = eng.bgzf_inflate(blob, np.array([off[0], o, off[2], off[3]]), cap_bytes=total, check=False)
        assert list(got["status"][:2]) == [-9, 1] and got["guard_intact"]
        check_others(got, good_payloads, {1})
    lim = off + np.array([len(b) for b in good])
    lim[2] -= 1
    got = eng.bgzf_inflate(blob, off, blk_limit=lim, cap_bytes=total, check=False)
    assert list(got["status"][:2]) == [-9, 2] and got["guard_intact"]
    got = eng.bgzf_inflate(blob[:-1], off, cap_bytes=total, check=False)
    assert list(got["status"][:2]) == [-9, 3] and got["guard_intact"]
    blob2, off2 = _place([good[0], bad["CRC32 mismatch"], good[1], bad["block type 3"]], [0, 1, 2, 3])
    got = eng.bgzf_inflate(blob2, off2, cap_bytes=70000, check=False)
    assert list(got["status"][:2]) == [-9, 1]
    # capacity: one byte short is PLAT_ERR_OVERFLOW at the block that does not fit, and no payload byte is written; a block error wins over it
    for cap, who in ((total - 1, 3), (len(good_payloads[0]) + 10, 1), (0, 0)):
        got = eng.bgzf_inflate(blob, off, cap_bytes=cap, check=False)
        assert list(got["status"]) == [-8, who, total, 0] and got["guard_intact"], cap
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            eng.bgzf_inflate(blob, off, cap_bytes=cap)
        assert e.value.code == -8
    got = eng.bgzf_inflate(blob2, off2, cap_bytes=10, check=False)
    assert list(got["status"][:2]) == [-9, 1] and got["guard_intact"]
    ok = eng.bgzf_inflate(blob, off, cap_bytes=total)
    assert list(ok["status"]) == [0, -1, total, 0] and ok["guard_intact"] and ok["data"].tobytes() == b"".join(good_payloads)


def _stream_case(data, first, stop, block_payload, blk0):
    """(BGZF blocks, chunk tuple) of one walk case whose blocks start at index blk0 of the call."""
    stream, off = synth.bgzf_stream(data, block_payload=block_payload, eof=False)
    n = len(off)
    sb, su = (-1, 0) if stop is None or stop >= len(data) else (blk0 + stop // block_payload, stop % block_payload)
    return stream, off, (blk0, blk0 + n, first, sb, su)


def test_record_walk_on_the_device():
    eng = H.get_engine()
    cases = K.walk_cases()
    for bp in (65536, 100, 37):
        want = [K.rule_walk(d, f, s, t, b, e) for _, d, f, s, t, b, e in cases]
        good = [i for i, w in enumerate(want) if w[0] == 0]
        # every good case a stream of one call
        blobs, offs, streams, at, blk = [], [], [], 0, 0
        for i in good:
            _, d, f, s, t, b, e = cases[i]
            stream, off, chunk = _stream_case(d, f, s, bp, blk)
            blobs.append(stream); offs += [at + int(o) for o in off]
            at += len(stream); blk += len(off)
            streams.append((t, b, e, [chunk]))
        inf = eng.bgzf_inflate(b"".join(blobs), np.array(offs, dtype=np.int64), keep_device=True)
        assert inf["guard_intact"] and int(inf["status"][0]) == 0
        got = eng.bam_find_records(inf, streams)
        assert got["guard_intact"] and list(got["status"][:2]) == [0, -1]
        assert int(got["status"][2]) == sum(len(want[i][1]) for i in good) and int(got["status"][3]) == sum(want[i][2] for i in good)
        data = inf["data"].tobytes()
        for k, i in enumerate(good):
            base = int(inf["out_off"][streams[k][3][0][0]])
            a, z = got["stream_begin"][k], got["stream_begin"][k + 1]
            assert [int(o) - base for o in got["rec_off"][a:z]] == want[i][1], (cases[i][0], bp)
            for o, lim in zip(got["rec_off"][a:z], got["rec_limit"][a:z]):
                assert int(lim) == int(o) + struct.unpack_from("<i", data, int(o) - 4)[0]
        # no room, and one record short: PLAT_ERR_OVERFLOW, nothing written behind the capacity, the kept count still whole
        for cap in (0, int(got["status"][2]) - 1):
            short = eng.bam_find_records(inf, streams, cap_records=cap, check=False)
            assert int(short["status"][0]) == -8 and int(short["status"][2]) == int(got["status"][2]) and short["guard_intact"]
            assert int(short["stream_begin"][-1]) == cap
        # every bad case between two good streams: status names it, the good streams' counts stand
        for i, w in enumerate(want):
            if w[0] == 0:
                continue
            _, d, f, s, t, b, e = cases[i]
            g = cases[good[0]]
            parts = [_stream_case(g[1], g[2], g[3], bp, 0)]
            parts.append(_stream_case(d, f, s, bp, len(parts[0][1])))
            parts.append(_stream_case(g[1], g[2], g[3], bp, len(parts[0][1]) + len(parts[1][1])))
            offs, at = [], 0
            for stream, off, _ in parts:
                offs += [at + int(o) for o in off]
                at += len(stream)
            inf2 = eng.bgzf_inflate(b"".join(p[0] for p in parts), np.array(offs, dtype=np.int64), keep_device=True)
            st = [(g[4], g[5], g[6], [parts[0][2]]), (t, b, e, [parts[1][2]]), (g[4], g[5], g[6], [parts[2][2]])]
            bad = eng.bam_find_records(inf2, st, check=False)
            assert list(bad["status"][:2]) == [-9, 1] and bad["guard_intact"], (cases[i][0], bp)
            with pytest.raises(_lib.PlatypusDeviceError) as err:
                eng.bam_find_records(inf2, st)
            assert err.value.code == -9 and "stream 1" in str(err.value)
    # a stream of two chunks: the kept records of chunk 0, then chunk 1; a record outside the window in chunk 0 ends chunk 1 too
    M = [(0, 20)]
    c0 = b"".join(K.record(3, 1100 + 10 * k, M) for k in range(5))
    c1 = b"".join(K.record(3, 1200 + 10 * k, M) for k in range(4))
    ends = c0 + K.record(3, 5000, M)
    for first, want_kept in ((c0, 9), (ends, 5)):
        s0, o0 = synth.bgzf_stream(first, block_payload=90, eof=False)
        s1, o1 = synth.bgzf_stream(c1, block_payload=90, eof=False)
        inf = eng.bgzf_inflate(s0 + s1, np.concatenate([o0, o1 + len(s0)]), keep_device=True)
        got = eng.bam_find_records(inf, [(3, 1000, 2000, [(0, len(o0), 0, -1, 0), (len(o0), len(o0) + len(o1), 0, -1, 0)])])
        assert list(got["status"][:3]) == [0, -1, want_kept] and list(got["stream_begin"]) == [0, want_kept]
        assert np.all(np.diff(got["rec_off"]) > 0)
    # an empty call
    inf = eng.bgzf_inflate(b"", np.zeros(0, np.int64), keep_device=True)
    got = eng.bam_find_records(inf, [])
    assert list(got["status"]) == [0, -1, 0, 0] and list(got["stream_begin"]) == [0]


def _cases():
    with gzip.open(os.path.join(HERE, "golden", "region_fetched_cases.json.gz"), "rt") as f:
        return json.load(f)


def _rule_end(pos, flag, cigar):
    """bam_endpos as plat_bam_decode_batch states it; `pos` is the read's (soft-clip-adjusted) position."""
    rec_pos = pos + (cigar[0][1] if cigar and cigar[0][0] == 4 else 0)
    if (flag & 4) or not cigar:
        return rec_pos + 1
    return rec_pos + sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))


def _itr_span(r):
    """(tid, b, e) of a read's record by the walk's rule (flag 4 plays no part)."""
    b = r.pos + (r.cigarOps[0][1] if r.cigarOps and r.cigarOps[0][0] == 4 else 0)
    return r.chromID, b, b + (sum(ln for op, ln in r.cigarOps if op in (0, 2, 3, 7, 8)) if r.cigarOps else 1)


def _decoy(tid, pos, n=50):
    return H.AlignedRead(b"A" * n, bytes([20] * n), pos, 30, 3, cigarOps=[(0, n)], chromID=tid, mateChromID=tid, insertSize=0, matePos=pos)


def _bam_and_bgzf(chrom, start, end, fasta, samples, **bgzf_kw):
    """One region for both calls.  The window is the smallest every fetched read passes; the decoys fail it: in front the same tid ending
    at or before itr_beg (two of them, one touching: e == itr_beg), behind the same tid with pos >= itr_end -- where the walk ends -- and
    then a lower tid, which is never read.  (A lower tid in FRONT would end the walk by the same rule, as the walk cases show; a
    coordinate-sorted file has none there.)"""
    spans = [_itr_span(r) for fetched, _ in samples for r in fetched]
    tid = spans[0][0] if spans else 0
    beg, stop = (min(e for _, _, e in spans) - 1, max(b for _, b, _ in spans) + 1) if spans else (start, end)
    front = [_decoy(tid, beg - 200), _decoy(tid, beg - 50)]
    behind = [_decoy(tid, stop), _decoy(tid, stop + 30), _decoy(tid - 1, beg + 10)]
    # by the rule, restated: every fetched read passes this window, every decoy fails it
    passes = lambda t, b, e: t == tid and b < stop and e > beg
    assert all(passes(*s) for s in spans)
    assert not any(passes(*_itr_span(d)) for d in front + behind)
    bam = F.BamRegion.from_reads(chrom, start, end, fasta, samples, lead=1, block_size=True)
    bgz = F.BgzfRegion.from_reads(chrom, start, end, fasta, samples, decoys=(front, behind), itr=(tid, beg, stop), **bgzf_kw)
    return bam, bgz


def test_bgzf_region_loop_equals_the_bam_loop_on_all_cases():
    """All 41 cases of the fetched fixture through plat_call_bgzf_regions -- each sample's reads as records, as a BGZF stream with decoy
    records in front and behind, in one or two chunks, blocks of 65 280, 4 000 or 700 bytes at levels 1, 6 and 9: text, rlen, loaded,
    per-sample counts and region text lengths are those of plat_call_bam_regions on the same records without decoys; input_bytes is the
    compressed bytes and smaller than the BAM call's -- wherever the BAM call uploads a byte: in two of the 41 cases no loaded region holds
    a read, the BAM call's input_bytes is 0, and the test asserts exactly that instead."""
    from tests.region_golden import _reads
    cases = _cases()
    with gzip.open(os.path.join(HERE, "golden", "region_cases.json.gz"), "rt") as f:
        after = json.load(f)
    assert len(cases) == 41
    nc = F.NativeCaller(0, 2, 2)
    n_lines = n_skipped = spanning = two_chunks = n_empty = 0
    sizes = []
    try:
        for ci, (case, ref) in enumerate(zip(cases, after)):
            fasta = H.FastaFile({"20": case["ref"].encode()})
            bam, bgz = [], []
            for r, rr in zip(case["regions"], ref["regions"]):
                samples = []
                for i, s in enumerate(r["samples"]):
                    fr = [K.aligned(x, _rule_end(x["pos"], x["flag"], x["cigar"])) for x in s["fetched"]]
                    br = _reads(rr["samples"][i]["brokenMates"]) if rr["loaded"] else []
                    for b in br:
                        b.end = _rule_end(b.pos, b.bitFlag, b.cigarOps)
                    samples.append((fr, br))
                a, z = _bam_and_bgzf(r["chrom"], r["start"], r["end"], fasta, samples, level=(1, 6, 9)[ci % 3], block_payload=(0xff00, 4000, 700)[ci % 3],
                                     n_chunks=1 + ci % 2)
                bam.append(a); bgz.append(z)
                spanning += z.made["records_spanning_blocks"]
                two_chunks += z.made["chunks"] == 2
            o1, o2 = default_options(**case["options"]), default_options(**case["options"])
            want = nc.call_bam_regions(bam, case["sample_names"], o1)
            want_loaded, want_counts, want_lens, bam_bytes = list(nc.loaded), nc.read_counts.copy(), nc.region_text_lengths(len(bam)).copy(), nc.stats["input_bytes"]
            got = nc.call_bgzf_regions(bgz, case["sample_names"], o2)
            assert got == want, ci
            assert o2.rlen == o1.rlen, ci
            assert nc.loaded == want_loaded == [int(r["loaded"]) for r in case["regions"]], ci
            assert np.array_equal(nc.read_counts, want_counts), ci
            assert np.array_equal(nc.region_text_lengths(len(bgz)), want_lens), ci
            compressed = sum(reg.compressed_bytes + sum(len(b[0]) for _, b in reg.samples if len(b[1])) for k, reg in enumerate(bgz) if want_loaded[k])
            sizes.append((ci, nc.stats["input_bytes"], bam_bytes))
            print("case %d: input_bytes bgzf %d, bam %d" % sizes[-1])
            assert nc.stats["input_bytes"] == compressed, ci
            if bam_bytes:
                assert nc.stats["input_bytes"] < bam_bytes, sizes[-1]
            else:                                                         # (cases 16 and 19: no read in a loaded region, so the BAM call uploads nothing and
                n_empty += 1                                              #  nothing can be smaller; what the BGZF call uploads there is its decoys' blocks)
                assert not any(len(s["fetched"]) for k, r in enumerate(case["regions"]) if want_loaded[k] for s in r["samples"]), ci
            n_lines += got.count("\n")
            n_skipped += want_loaded.count(0)
    finally:
        nc.close()
    # a record split across blocks, a fetch of two chunks, and the maxReads bail-out through the kept counts (the decoys are not counted:
    # loaded equals the BAM call's, whose counts hold no decoy)
    assert spanning >= 1 and two_chunks >= 1 and n_skipped >= 1 and n_lines > 200 and n_empty <= 2


def _rule_ends(reads):
    import copy
    out = copy.deepcopy(reads)
    for r in out:
        r.end = _rule_end(r.pos, r.bitFlag, r.cigarOps)
    return out


def test_synthetic_regions_equal_the_bam_call():
    """The nine synthetic config-4 regions of the BAM test, 1-3 samples, at levels 1 and 6: text, counts and rlen of the BAM call."""
    groups = {1: [], 2: [], 3: []}
    for idx, nS in ((0, 1), (1, 2), (2, 1), (3, 3), (4, 2), (5, 1), (6, 3), (7, 2), (8, 1)):
        reg, samples = synth.config4_fetched_region(idx, region_len=20000, n_samples=nS)
        samples = [_rule_ends(rs) for rs in samples]
        fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
        pairs = [(rs, []) for rs in samples]
        both = [_bam_and_bgzf(reg["chrom"], reg["start"], reg["end"], fasta, pairs, level=lv, n_chunks=1 + idx % 2) for lv in (1, 6)]
        groups[nS].append((both[0][0], both[0][1], both[1][1]))
    nc = F.NativeCaller(0, 2, 2)
    try:
        for nS, regs in groups.items():
            nm = ["S%d" % (i + 1) for i in range(nS)]
            o1 = default_options()
            want = nc.call_bam_regions([r[0] for r in regs], nm, o1)
            counts, bam_bytes = nc.read_counts.copy(), nc.stats["input_bytes"]
            assert want.count("\n") > 5 and 0 < counts[:, :, 1].sum() < counts[:, :, 0].sum()
            for which in (1, 2):
                o2 = default_options()
                got = nc.call_bgzf_regions([r[which] for r in regs], nm, o2)
                assert got == want and o1.rlen == o2.rlen and np.array_equal(nc.read_counts, counts)
                assert nc.stats["input_bytes"] == sum(r[which].compressed_bytes for r in regs) < bam_bytes
    finally:
        nc.close()


def test_bad_blocks_and_chunks_are_refused_and_the_caller_stays_usable():
    ref = b"ACGTTGCA" * 100
    fasta = H.FastaFile({"20": ref})

    def reads(order):
        return [H.AlignedRead(ref[p:p + 60], bytes([30] * 60), p, bitFlag=3) for p in order]

    def region(order, **kw):
        return F.BgzfRegion.from_reads("20", 100, 500, fasta, [(reads(order), [])], **kw)

    def edited(reg, edit):
        chunks, broken = reg.samples[0]
        d, fu, ec, eu = chunks[0]
        d, fu, ec, eu = edit(bytearray(d.tobytes()), fu, ec, eu)
        return F.BgzfRegion("20", 100, 500, ref, reg.tid, reg.itr_beg, reg.itr_end, [([(bytes(d), fu, ec, eu)] + chunks[1:], broken)])

    order = [100, 140, 180, 200, 220, 260, 300]
    nc = F.NativeCaller(0, 1, 2)
    try:
        want = nc.call_bam_regions([F.BamRegion.from_reads("20", 100, 500, fasta, [(reads(order), [])])], ["S1"], default_options())
        good = region(order, block_payload=200)
        assert good.made["blocks"] >= 4 and nc.call_bgzf_regions([good], ["S1"], default_options()) == want
        data = good.samples[0][0][0][0].tobytes()
        second = struct.unpack_from("<H", data, 16)[0] + 1                         # (BSIZE + 1, the first block's length: where block 1 starts)
        assert data[second:second + 4] == b"\x1f\x8b\x08\x04"

        # a corrupt block inside a multi-region call: a CRC byte of block 1 of region 1
        def flip_crc(d, fu, ec, eu):
            end1 = second + struct.unpack_from("<H", d, second + 16)[0] + 1
            d[end1 - 8] ^= 0x40
            return d, fu, ec, eu
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bgzf_regions([region(order), edited(good, flip_crc), region(order)], ["S1"], default_options())
        msg = str(e.value)
        assert e.value.code == -9 and "region 1" in msg and "sample 0" in msg and "chunk 0" in msg and "block 1" in msg
        assert nc.call_bgzf_regions([good], ["S1"], default_options()) == want

        # a broken BSIZE chain: block 1's magic
        def break_chain(d, fu, ec, eu):
            d[second + 1] = 0x8c
            return d, fu, ec, eu
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bgzf_regions([region(order), edited(good, break_chain)], ["S1"], default_options())
        msg = str(e.value)
        assert e.value.code == -9 and "region 1" in msg and "sample 0" in msg and "chunk 0" in msg and "do not chain" in msg
        assert nc.call_bgzf_regions([good], ["S1"], default_options()) == want

        # an end_coffset off a block boundary
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bgzf_regions([edited(good, lambda d, fu, ec, eu: (d, fu, second + 1, 0))], ["S1"], default_options())
        msg = str(e.value)
        assert e.value.code == -9 and "region 0" in msg and "sample 0" in msg and "chunk 0" in msg and "block boundary" in msg
        # ... and one on it: the chunk ends where block 1 starts, the records behind are not read
        part = nc.call_bgzf_regions([edited(good, lambda d, fu, ec, eu: (d, fu, second, 0))], ["S1"], default_options())
        assert nc.loaded == [1] and 0 < int(nc.read_counts[0][0][0]) < len(order)
        del part

        # a record walk that fails: the stream cut inside a record (the last block dropped)
        def drop_last(d, fu, ec, eu):
            at, last = 0, 0
            while at < len(d) - 28:                                              # (the EOF block stays behind the cut)
                last = at
                at += struct.unpack_from("<H", d, at + 16)[0] + 1
            return d[:last], fu, ec, eu
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bgzf_regions([region(order), edited(region(order, block_payload=230), drop_last)], ["S1"], default_options())
        msg = str(e.value)
        assert e.value.code == -9 and "region 1" in msg and "sample 0" in msg and "record walk" in msg
        assert nc.call_bgzf_regions([good], ["S1"], default_options()) == want
    finally:
        nc.close()
