"""GPU tests of plat_bgzf_deflate_batch at the seams of its block kernel and of the kernels around it (tests/bgzf_deflate_cases.py:
seam_blocks, seam_fuzz, batch_cases -- tests/test_bgzf_deflate_cpu.py asserts what each reaches and pins the host twin to the restatement on
them): the restatement's bytes, offsets and status at both levels, the guards, a second call, the device's inflate over the device's output;
big calls before and after small ones on one engine; overflow past the scans' first round; and plat_caller_compress_text's second attempt
and its slices against the same call on the host twin."""
import contextlib
import gzip
import os
import time

import numpy as np
import pytest

from platypus_amd import fastcaller as F, hostapi as H
from tests import bgzf_deflate_cases as K

pytestmark = pytest.mark.gpu

SEAM_GROUPS, SEAM_GROUP, FUZZ_GROUP = 4, 17, 50


@contextlib.contextmanager
def _host_deflate():
    old = os.environ.get("PLAT_CALLER_HOST_DEFLATE")
    os.environ["PLAT_CALLER_HOST_DEFLATE"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["PLAT_CALLER_HOST_DEFLATE"]
        else:
            os.environ["PLAT_CALLER_HOST_DEFLATE"] = old


def _device_is_the_restatement(eng, name, text, off, levels=(0, 1), again=True):
    for lv in levels:
        want, woff, sizes = K.compress(text, off, lv)
        got = eng.bgzf_deflate(text, off, level=lv)
        data = got["data"].tobytes()
        assert list(got["status"]) == [0, -1, len(want), len(sizes)], (name, lv)
        if data != want:                                                   # (name the first block that differs, not 60 KB of bytes)
            at = next(i for i in range(min(len(data), len(want))) if data[i] != want[i]) if len(data) == len(want) else min(len(data), len(want))
            blk = max(i for i, (a, _, _, _) in enumerate(K.parse_blocks(want)) if a <= at)
            raise AssertionError("%s, level %d: byte %d (block %d of %d) differs from the restatement's" % (name, lv, at, blk, len(sizes)))
        assert list(got["piece_out_off"]) == woff and got["guard_intact"], (name, lv)
        if again:
            second = eng.bgzf_deflate(text, off, level=lv)
            assert second["data"].tobytes() == data and list(second["status"]) == list(got["status"]) and second["guard_intact"], (name, lv)
            assert list(second["piece_out_off"]) == woff, (name, lv)
        if data and again:
            blk = np.array([a for a, _, _, _ in K.parse_blocks(data)], dtype=np.int64)
            back = eng.bgzf_inflate(data, blk)
            assert list(back["status"]) == [0, -1, len(text), 0] and back["guard_intact"], (name, lv)
            assert back["data"].tobytes() == text, (name, lv)


@pytest.mark.parametrize("group", range(SEAM_GROUPS))
def test_seam_blocks_are_the_restatements(group):
    eng = H.get_engine()
    assert SEAM_GROUP * (SEAM_GROUPS - 1) < len(K.seam_blocks()) <= SEAM_GROUP * SEAM_GROUPS
    for name, text, off in K.seam_blocks()[SEAM_GROUP * group:SEAM_GROUP * (group + 1)]:
        _device_is_the_restatement(eng, name, text, off)


@pytest.mark.parametrize("group", range(300 // FUZZ_GROUP))
def test_seam_fuzz_is_the_restatements(group):
    eng = H.get_engine()
    cases = K.seam_fuzz()
    assert len(cases) == 300
    for name, text, off in cases[FUZZ_GROUP * group:FUZZ_GROUP * (group + 1)]:
        _device_is_the_restatement(eng, name, text, off)


@pytest.mark.parametrize("index", range(5))
def test_batch_cases_are_the_restatements(index):
    _device_is_the_restatement(H.get_engine(), *K.batch_cases()[index])


def test_big_calls_before_and_after_small_ones():
    """One engine, both orders: the scratch a big call leaves (piece_blk, the block table, the words, the slots) is met by small calls,
    and the other way round."""
    eng = H.get_engine()
    big, small = K.batch_cases()[:2] + K.batch_cases()[3:4], K.seam_blocks()[::5] + K.seam_fuzz()[::40]
    for order in (big + small + big, small + big + small):
        for name, text, off in order:
            _device_is_the_restatement(eng, name, text, off, levels=(1,), again=False)
    _device_is_the_restatement(eng, *K.batch_cases()[0], levels=(0,), again=False)
    _device_is_the_restatement(eng, *K.seam_blocks()[0])


@pytest.mark.parametrize("index, pieces", [(3, (4100, 4500, 8191, 8192, 8999)), (0, (1025, 1050, 1099))])
def test_overflow_past_the_scans_first_round(index, pieces):
    """Capacities one byte short of a piece boundary behind piece 4096 (9000 pieces) and behind piece 1024 (1100 pieces): the first piece
    that does not fit, the size needed, clamped offsets, not a byte written; then success at the size named."""
    eng = H.get_engine()
    name, text, off = K.batch_cases()[index]
    want, woff, sizes = K.compress(text, off, 1)
    assert len(woff) - 1 > max(pieces) and (index != 3 or len(sizes) > 8192)
    for i in pieces:
        cap = woff[i + 1] - 1
        first = next(k for k in range(len(woff) - 1) if woff[k + 1] > cap)
        assert first <= i and (first == i or woff[first + 1] == woff[i + 1]) and first > (4096 if index == 3 else 1024)
        got = eng.bgzf_deflate(text, off, level=1, cap_bytes=cap, check=False)
        assert list(got["status"]) == [-8, first, len(want), len(sizes)], (name, i)
        assert got["guard_intact"] and len(got["data"]) == 0, (name, i)
        assert list(got["piece_out_off"]) == [min(x, cap) for x in woff], (name, i)
    got = eng.bgzf_deflate(text, off, level=1, cap_bytes=int(got["status"][2]))
    assert got["data"].tobytes() == want and got["guard_intact"] and list(got["status"]) == [0, -1, len(want), len(sizes)]


def test_compress_text_asks_twice_when_five_eighths_are_too_little():
    """200 KB of random printable bytes in 5 regions deflate to more than 5/8 of their length plus 4096: the first attempt overflows and
    the second, at the size the device named, gives the twin's bytes."""
    rng = np.random.default_rng(20264)
    text = bytes(rng.integers(33, 127, size=200_000, dtype=np.uint8))
    lens = np.array([70_000, 1, 0, 129_000, 999], dtype=np.int64)
    off = [0] + [int(x) for x in np.cumsum(lens)]
    want, woff, _ = K.compress(text, off, 1)
    assert int(lens.sum()) == len(text) and len(want) > len(text) // 8 * 5 + 4096          # (the first capacity of host/bgzf_out.hpp)
    nc = F.NativeCaller(0, 1, 1)
    try:
        z, zl = nc.compress_text(text, lens, eof=False)
        with _host_deflate():
            hz, hzl = nc.compress_text(text, lens, eof=False)
        z = bytes(z)
        assert z == bytes(hz) == want and list(zl) == list(hzl) == list(np.diff(woff))
        assert gzip.decompress(z) == text
        z0, zl0 = nc.compress_text(text, lens, level=0)
        assert bytes(z0) == K.compress(text, off, 0)[0] + K.EOF_BLOCK and int(zl0.sum()) == len(z0) - 28
    finally:
        nc.close()


def test_compress_text_in_slices_on_two_workers():
    """Regions of 20 MiB, 12 MiB, 1, 0 and 33 MiB: the first two fill a slice of 32 MiB exactly, the next two are a slice, the last is
    longer than a slice and sits alone.  Two workers take them; the bytes and the per-region lengths are the twin's."""
    MiB = 1 << 20
    lens = np.array([20 * MiB, 12 * MiB, 1, 0, 33 * MiB], dtype=np.int64)
    rng = np.random.default_rng(20265)
    lines = [b"chr20\t%d\t.\t%s\t%s\t%d\tPASS\tDP=%d;TC=%d\tGT:GL:GQ:NR:NV\t%s:-%d.%d,0,-%d.0:%d:%d:%d\n" % (
        1000 + 37 * i, b"ACGT"[i % 4:i % 4 + 1], b"TGCA"[i % 3:i % 3 + 1], 20 + i % 80, i % 50, i % 61, (b"0/1", b"1/1")[i & 1], i % 90, i % 10, i % 70, i % 99, i % 40, i % 17)
        for i in range(256)]
    pool = np.frombuffer(b"".join(lines[i] for i in rng.integers(0, len(lines), size=16_000)), dtype=np.uint8)
    assert MiB < len(pool) < 2 * MiB
    text = np.resize(pool, int(lens.sum()))
    nc = F.NativeCaller(0, 2, 2)
    try:
        t0 = time.time()
        z, zl = nc.compress_text(text, lens)
        t1 = time.time()
        with _host_deflate():
            hz, hzl = nc.compress_text(text, lens)
        t2 = time.time()
        print("compress_text of %d MiB in 3 slices: the device %.2f s, the host twin %.2f s, %d -> %d bytes" % (
            len(text) // MiB, t1 - t0, t2 - t1, len(text), len(z)))
        zb, hzb = np.frombuffer(z, dtype=np.uint8), np.frombuffer(hz, dtype=np.uint8)
        assert list(zl) == list(hzl) and int(zl.sum()) == len(zb) - 28 and zl[3] == 0 and zl[2] == 18 + 3 + 8
        assert np.array_equal(zb, hzb)
        back = gzip.decompress(zb)
        assert len(back) == len(text) and np.array_equal(np.frombuffer(back, dtype=np.uint8), text)
        # a region begins on a block boundary, and the EOF block ends it all
        at = int(zl[:4].sum())
        assert zb[at:at + 4].tobytes() == b"\x1f\x8b\x08\x04" and zb[-28:].tobytes() == K.EOF_BLOCK
        blocks = lambda n: (n + K.PAYLOAD - 1) // K.PAYLOAD
        head = K.parse_blocks(zb[:int(zl[0])].tobytes())
        assert len(head) == blocks(20 * MiB) and head[-1][2] == 20 * MiB - (blocks(20 * MiB) - 1) * K.PAYLOAD
    finally:
        nc.close()
