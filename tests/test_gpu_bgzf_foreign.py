"""GPU tests of plat_bgzf_inflate_batch and plat_bam_find_records on input that zlib's encoder never writes: the streams of
tests/deflate_writer.py (bgzf_cases.foreign_blocks / foreign_fuzz -- codes of up to 15 bits through the canonical walk, the headers'
full ranges, matches placed on the seams of the wave's replay, far edges, block sequences) and the record walk's window-seam ladder
(bgzf_cases.walk_seam_cases).  Every verdict and payload is zlib's (bgzf_cases.reference_verdict), every record list rule_walk's.  The
device sees only inputs the sanitized host build of the same code has handled first (tests/test_bgzf_cpu.py); the refusals exercise
error returns and none provokes a fault."""
import struct

import numpy as np
import pytest

from platypus_amd import hostapi as H, synth
from tests import bgzf_cases as K

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def verdicts():
    """(valid [(name, payload, block)], refused [(name, block)]) over the named cases, the fuzz streams and their flipped copies."""
    fuzz, _ = K.foreign_fuzz()
    every = [(n, b) for n, _, b in K.foreign_blocks()] + [(n, b) for n, _, b, _ in fuzz] + [(n + ", flipped", f) for n, _, _, f in fuzz]
    valid, refused = [], []
    for name, block in every:
        v = K.reference_verdict(block)
        if v is None:
            refused.append((name, block))
        else:
            valid.append((name, v, block))
    assert len(valid) >= 630 and len(refused) >= 300
    return valid, refused


def test_valid_foreign_streams_in_one_call(verdicts):
    eng = H.get_engine()
    valid, _ = verdicts
    blocks, payloads = [b for _, _, b in valid], [p for _, p, _ in valid]
    gaps = [(3, 1, 2, 5, 0, 7)[i % 6] for i in range(len(blocks))]
    blob, off = _place(blocks, gaps)
    assert all(sum(1 for o in off if int(o) & 3 == a) > 100 for a in range(4))       # all four byte alignments
    total = sum(len(p) for p in payloads)
    want_off = [0] + list(np.cumsum([len(p) for p in payloads]))
    for lim in (None, off + np.array([len(b) for b in blocks])):                      # ... and with each block's own end as its limit
        got = eng.bgzf_inflate(blob, off, blk_limit=lim, check=False)
        data = got["data"].tobytes()
        wrong = [valid[i][0] for i, p in enumerate(payloads) if data[want_off[i]:want_off[i] + len(p)] != p]
        assert list(got["status"]) == [0, -1, total, 0], (got["status"], valid[int(got["status"][1])][0])
        assert list(got["out_off"]) == want_off
        assert wrong == []
        assert got["guard_intact"]


def test_refused_foreign_streams_one_to_a_call(verdicts):
    eng = H.get_engine()
    valid, refused = verdicts
    good_payloads = [b"in front of it " * 40, K.synthetic_record_bytes(5000)]
    good = [synth.bgzf_block(p, lv) for p, lv in zip(good_payloads, (6, 1))]
    cap = sum(len(p) for p in good_payloads) + 65536
    not_refused, neighbours, guards = [], [], []
    for k, (name, block) in enumerate(refused):
        blob, off = _place([good[0], block, good[1]], [k % 4, 1 + k % 3, k % 5])
        lim = off + np.array([len(good[0]), len(block), len(good[1])])
        got = eng.bgzf_inflate(blob, off, blk_limit=lim, cap_bytes=cap, check=False)
        if list(got["status"][:2]) != [-9, 1]:
            not_refused.append((name, list(got["status"])))
        data = got["data"].tobytes()
        for i in (0, 2):
            a = int(got["out_off"][i])
            if data[a:a + len(good_payloads[i // 2])] != good_payloads[i // 2]:
                neighbours.append(name)
        if not got["guard_intact"]:
            guards.append(name)
    assert not_refused == [] and neighbours == [] and guards == []
    # a good call afterwards: the named valid cases again
    blocks, payloads = [b for _, _, b in valid[:100]], [p for _, p, _ in valid[:100]]
    blob, off = _place(blocks, [2] * len(blocks))
    ok = eng.bgzf_inflate(blob, off)
    assert list(ok["status"]) == [0, -1, sum(len(p) for p in payloads), 0] and ok["guard_intact"] and ok["data"].tobytes() == b"".join(payloads)


def _check_walk(inf, got, cases, want, chunks, tag):
    data = inf["data"].tobytes()
    assert got["guard_intact"] and list(got["status"][:2]) == [0, -1], tag
    assert int(got["status"][2]) == sum(len(w[1]) for w in want) and int(got["status"][3]) == sum(w[2] for w in want), tag
    assert list(got["stream_begin"]) == [0] + list(np.cumsum([len(w[1]) for w in want])), tag
    for k, (case, w) in enumerate(zip(cases, want)):
        base = int(inf["out_off"][chunks[k][0]])
        a, z = got["stream_begin"][k], got["stream_begin"][k + 1]
        assert [int(o) - base for o in got["rec_off"][a:z]] == w[1], (case[0], tag)
        assert [int(x) for x in got["rec_limit"][a:z]] == [int(o) + struct.unpack_from("<i", data, int(o) - 4)[0] for o in got["rec_off"][a:z]], (case[0], tag)


def test_window_seam_ladder_on_the_device():
    eng = H.get_engine()
    cases, probes = K.walk_seam_cases()
    want = [K.rule_walk(d, f, s, t, b, e) for _, d, f, s, t, b, e in cases]
    assert all(w[0] == 0 for w in want)
    for bp in (65536, 37):
        made = [synth.bgzf_stream(d, block_payload=bp, eof=False) for _, d, *_ in cases]
        # one stream per call: every stream's bytes start at offset 0, where the case file's window bases hold
        for case, w, (stream, off) in zip(cases, want, made):
            inf = eng.bgzf_inflate(stream, off, keep_device=True)
            chunk = (0, len(off), case[2], -1, 0)
            got = eng.bam_find_records(inf, [(case[4], case[5], case[6], [chunk])])
            _check_walk(inf, got, [case], [w], [chunk], (bp, "alone"))
        # all streams in one call: the ladder's streams are multiples of 4 long and come first, so their bases hold here too; behind them the
        # streams of other lengths lie at all alignments, the bytes behind one stream's end being the next stream's
        assert all(len(cases[i][1]) % 4 == 0 for i in probes) and max(probes) == len(probes) - 1
        assert {sum(len(c[1]) for c in cases[:k]) % 4 for k in range(len(probes), len(cases))} == {0, 1, 2, 3}
        offs, chunks, at, blk = [], [], 0, 0
        for case, (stream, off) in zip(cases, made):
            offs += [at + int(o) for o in off]
            chunks.append((blk, blk + len(off), case[2], -1, 0))
            at += len(stream)
            blk += len(off)
        inf = eng.bgzf_inflate(b"".join(s for s, _ in made), np.array(offs, dtype=np.int64), keep_device=True)
        assert inf["guard_intact"] and inf["data"].tobytes() == b"".join(c[1] for c in cases)
        streams = [(c[4], c[5], c[6], [ch]) for c, ch in zip(cases, chunks)]
        got = eng.bam_find_records(inf, streams)
        _check_walk(inf, got, cases, want, chunks, (bp, "together"))
        # one record of capacity short: PLAT_ERR_OVERFLOW with the full count, nothing written behind the capacity
        kept = int(got["status"][2])
        short = eng.bam_find_records(inf, streams, cap_records=kept - 1, check=False)
        assert int(short["status"][0]) == -8 and int(short["status"][2]) == kept and int(short["status"][3]) == int(got["status"][3])
        assert short["guard_intact"] and int(short["stream_begin"][-1]) == kept - 1
        assert list(short["rec_off"]) == list(got["rec_off"][:kept - 1])
