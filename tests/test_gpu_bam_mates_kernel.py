"""GPU tests of plat_bam_mates_batch (include/platypus_mi355x.h, csrc/plat_bammates.hip) against a Python restatement of
csrc/mate_rule.hpp over the records' bytes (struct.unpack): one batch whose streams hold 0, 1, 63, 64, 65, 255, 256, 257 and 1000 records
-- wave and tile seams, a stream of several tiles, empty streams at the front, in the middle and at the end --, read names of every
length 1..16 (refID on every alignment mod 16), every combination of flags 0x2 / 0x4 / 0x8 with mtid in {-1, tid, other}, a first wave
of records that pass neither rule; both modes; the capacities one short; and a record shorter than its fixed fields."""
import struct

import numpy as np
import pytest

from platypus_amd import hostapi as H

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 0, 64, 65, 255, 256, 257, 1000, 0]
TID, OTHER, LO, HI = 3, 1, 5000, 6000
PAD = 32


def _record(i, flag, mtid, mpos):
    """One alignment record from refID on: a name of 1..16 bytes (NUL included), a 1-op CIGAR, i % 40 + 1 bases, now and then aux data."""
    name = bytes(97 + (i + k) % 26 for k in range(i % 16)) + b"\0"
    n = i % 40 + 1
    aux = b"RGZg%d\0" % (i % 7) if i % 3 == 0 else b""
    return (struct.pack("<iiBBHHHiiii", TID, 100 + i, len(name), 60, 0, 1, flag, n, mtid, mpos, 0) + name + struct.pack("<I", n << 4) +
            bytes([0x12 + (i & 1)] * ((n + 1) // 2)) + bytes([(30 + i) % 60] * n) + aux)


@pytest.fixture(scope="module")
def batch():
    """(blob, rec_off, rec_limit, stream_begin, per-stream (want_tid, lo, hi)) -- a 4-byte block_size in front of every record, as an
    inflated stream holds them, and a 5-byte lead so that the first refID is unaligned too."""
    rng = np.random.default_rng(522)
    parts, off, lim, begin, at, i = [b"\xa5" * 5], [], [], [0], 5, 0
    for s, size in enumerate(SIZES):
        for j in range(size):
            if s in (1, 2):                                                     # records 0..63, the batch's first wave: proper pairs whose mates lie elsewhere
                flag, mtid, mpos = 0x43, OTHER, 77
            else:
                flag = int(rng.choice([0, 2, 4, 6, 8, 10, 12, 14])) | int(rng.choice([1, 0x41, 0x81, 0x411]))
                mtid = TID if s == 4 else int(rng.choice([-1, TID, TID, OTHER]))       # (stream 4: every mate on the region's contig)
                mpos = int(rng.choice([LO - 1, LO, HI, HI + 1, int(rng.integers(LO - 300, HI + 300)), int(rng.integers(0, 1 << 30))]))
            rec = _record(i, flag, mtid, mpos)
            parts.append(struct.pack("<i", len(rec)) + rec)
            off.append(at + 4)
            lim.append(at + 4 + len(rec))
            at += 4 + len(rec)
            i += 1
        begin.append(len(off))
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8)
    n = len(SIZES)
    assert {o % 16 for o in off} == set(range(16))
    # stream 4 keeps everything, stream 5 nothing; the others the region's own filter
    want = np.full(n, TID, dtype=np.int32)
    lo, hi = np.full(n, LO, dtype=np.int32), np.full(n, HI, dtype=np.int32)
    lo[4], hi[4] = -(1 << 31), (1 << 31) - 1
    want[5] = 9
    return blob, np.array(off, dtype=np.int64), np.array(lim, dtype=np.int64), np.array(begin, dtype=np.int32), (want, lo, hi)


def _fields(blob, off):
    flag = struct.unpack_from("<H", blob, off + 14)[0]
    mtid, mpos = struct.unpack_from("<ii", blob, off + 20)
    return flag, mtid, mpos


def _restate(batch, mode):
    """Per stream the kept records' indices, by the rule."""
    blob, off, lim, begin, (want, lo, hi) = batch
    raw = blob.tobytes()
    kept = []
    for s in range(len(begin) - 1):
        here = []
        for i in range(begin[s], begin[s + 1]):
            flag, mtid, mpos = _fields(raw, int(off[i]))
            if mode == "coords":
                ok = (not (flag & 2) or bool(flag & 4) or bool(flag & 8)) and mtid != -1
            else:
                ok = mtid == want[s] and lo[s] <= mpos <= hi[s]
            if ok:
                here.append(i)
        kept.append(here)
    return kept


def test_coords_of_every_stream_equal_the_restatement(batch):
    eng = H.get_engine()
    blob, off, lim, begin, _ = batch
    kept = _restate(batch, "coords")
    flat = [i for k in kept for i in k]
    assert kept[1] == kept[2] == [] and int(begin[3]) == 64 and all(0 < len(kept[s]) < SIZES[s] for s in (4, 5, 6, 7, 8, 9))      # (the first wave passes nothing)
    got = eng.bam_mates(blob, off, lim, begin, "coords")
    assert list(got["status"]) == [0, -1, len(flat), int(begin[-1])]
    assert list(got["begin"]) == [0] + list(np.cumsum([len(k) for k in kept]))
    raw = blob.tobytes()
    assert got["coords"].tolist() == [list(_fields(raw, int(off[i]))[1:]) for i in flat]
    assert got["guard_intact"]
    # the capacity of the find, larger than the records: what lies behind stream_begin[-1] is not looked at
    more = eng.bam_mates(blob, np.append(off, [-5] * 9), np.append(lim, [1 << 40] * 9), begin, "coords", n_records=len(off) + 9, cap_records=len(flat))
    assert list(more["status"]) == list(got["status"]) and more["coords"].tolist() == got["coords"].tolist() and more["guard_intact"]


def test_fetch_copies_the_mates_of_every_stream(batch):
    eng = H.get_engine()
    blob, off, lim, begin, (want, lo, hi) = batch
    kept = _restate(batch, "fetch")
    flat = [i for k in kept for i in k]
    assert kept[1] == kept[2] == [] and len(kept[4]) == SIZES[4] and kept[5] == [] and all(0 < len(kept[s]) < SIZES[s] for s in (6, 7, 8, 9))
    raw = blob.tobytes()
    recs = [raw[int(off[i]):int(lim[i])] for i in flat]
    got = eng.bam_mates(blob, off, lim, begin, "fetch", want, lo, hi)
    assert list(got["status"]) == [0, -1, len(flat), int(begin[-1])]
    assert got["need_bytes"] == sum(len(r) for r in recs)
    assert list(got["begin"]) == [0] + list(np.cumsum([len(k) for k in kept]))
    assert got["rec_len"].tolist() == [len(r) for r in recs]
    assert got["rec_off"].tolist() == [0] + list(np.cumsum([len(r) for r in recs]))[:-1]
    assert got["mpos"].tolist() == [_fields(raw, int(off[i]))[2] for i in flat]
    assert got["data"].tobytes() == b"".join(recs)
    assert {o % 16 for o in got["rec_off"].tolist()} == set(range(16)) and not got["pad"].any() and len(got["pad"]) == PAD
    assert got["guard_intact"]
    # exactly the room it needs
    tight = eng.bam_mates(blob, off, lim, begin, "fetch", want, lo, hi, cap_records=len(flat), cap_bytes=got["need_bytes"])
    assert list(tight["status"]) == list(got["status"]) and tight["data"].tobytes() == got["data"].tobytes() and tight["guard_intact"]


@pytest.mark.parametrize("short", ["records", "bytes"])
def test_a_capacity_one_short_is_an_overflow_with_full_counts(batch, short):
    eng = H.get_engine()
    blob, off, lim, begin, (want, lo, hi) = batch
    kept = _restate(batch, "fetch")
    flat = [i for k in kept for i in k]
    need = sum(int(lim[i] - off[i]) for i in flat)
    cap_r, cap_b = (len(flat) - 1, need) if short == "records" else (len(flat), need - 1)
    got = eng.bam_mates(blob, off, lim, begin, "fetch", want, lo, hi, cap_records=cap_r, cap_bytes=cap_b, check=False)
    last = max(s for s in range(len(kept)) if kept[s])                          # the stream of the one record that does not fit
    assert list(got["status"]) == [-8, last, len(flat), int(begin[-1])] and got["need_bytes"] == need
    assert got["guard_intact"]
    raw = blob.tobytes()
    assert got["rec_len"].tolist() == [int(lim[i] - off[i]) for i in flat[:-1]]
    assert got["data"].tobytes()[:need - int(lim[flat[-1]] - off[flat[-1]])] == b"".join(raw[int(off[i]):int(lim[i])] for i in flat[:-1])
    assert int(got["begin"][-1]) == cap_r
    if short == "records":
        c = _restate(batch, "coords")
        n = sum(len(k) for k in c)
        got = eng.bam_mates(blob, off, lim, begin, "coords", cap_records=n - 1, check=False)
        assert list(got["status"]) == [-8, max(s for s in range(len(c)) if c[s]), n, int(begin[-1])] and got["guard_intact"] and len(got["coords"]) == n - 1


def test_a_record_shorter_than_its_fixed_fields_refuses_only_its_stream(batch):
    eng = H.get_engine()
    blob, off, lim, begin, (want, lo, hi) = batch
    bad = int(begin[7]) + 70                                                     # a record of stream 7, behind its first wave
    lim2 = lim.copy()
    lim2[bad] = off[bad] + 31
    for mode in ("coords", "fetch"):
        kept = _restate(batch, mode)
        kept[7] = [i for i in kept[7] if i != bad]
        flat = [i for k in kept for i in k]
        got = eng.bam_mates(blob, off, lim2, begin, mode, want, lo, hi, check=False)
        assert list(got["status"]) == [-9, 7, len(flat), int(begin[-1])]
        assert list(got["begin"]) == [0] + list(np.cumsum([len(k) for k in kept])) and got["guard_intact"]
        raw = blob.tobytes()
        if mode == "coords":
            assert got["coords"].tolist() == [list(_fields(raw, int(off[i]))[1:]) for i in flat]
        else:
            assert got["data"].tobytes() == b"".join(raw[int(off[i]):int(lim[i])] for i in flat)
    # offsets outside the data, in front of it and behind it, name the lowest stream
    off3, lim3 = off.copy(), lim.copy()
    off3[int(begin[9]) + 5] = -4
    lim3[int(begin[4]) + 1] = len(blob) + 1
    got = eng.bam_mates(blob, off3, lim3, begin, "coords", check=False)
    assert list(got["status"][:2]) == [-9, 4] and got["guard_intact"]
    # a stream_begin that is no partition is refused whole
    broken = begin.copy()
    broken[3] = broken[2] - 1
    got = eng.bam_mates(blob, off, lim, broken, "coords", check=False)
    assert list(got["status"]) == [-1, -1, 0, 0] and not got["begin"].any() and got["guard_intact"]
