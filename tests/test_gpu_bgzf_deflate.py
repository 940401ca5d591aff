"""GPU tests of the compressed VCF output: plat_bgzf_deflate_batch against the host twin of its rule (csrc/bgzf_deflate.hpp, reached through
PLAT_CALLER_HOST_DEFLATE=1) and the rule's Python restatement on the cases both have passed on the CPU (tests/test_bgzf_deflate_cpu.py,
tests/bgzf_deflate_cases.py); the device's own inflate on the device's output; the overflow contract; plat_caller_compress_text on a
synthetic call's text; and the CLI writing x.vcf.gz."""
import gzip
import os

import numpy as np
import pytest

from platypus_amd import fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options
from tests import bgzf_deflate_cases as K

pytestmark = pytest.mark.gpu


class _HostDeflate:
    def __enter__(self):
        self.old = os.environ.get("PLAT_CALLER_HOST_DEFLATE")
        os.environ["PLAT_CALLER_HOST_DEFLATE"] = "1"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["PLAT_CALLER_HOST_DEFLATE"]
        else:
            os.environ["PLAT_CALLER_HOST_DEFLATE"] = self.old


@pytest.fixture(scope="module")
def twin():
    """{(case name, level): the host twin's bytes and per-piece lengths}, computed once."""
    out = {}
    nc = F.NativeCaller(0, 1, 1)
    try:
        with _HostDeflate():
            for name, text, off in K.cases():
                for lv in (0, 1):
                    z, zl = nc.compress_text(text, np.diff(np.asarray(off, dtype=np.int64)), level=lv, eof=False)
                    out[(name, lv)] = (bytes(z), [0] + [int(x) for x in np.cumsum(zl)])
    finally:
        nc.close()
    return out


@pytest.mark.parametrize("index", range(13))
def test_device_bytes_are_the_host_twins(index, twin):
    """Both levels of one case: the device's bytes, offsets and status against the twin's and the restatement's; the guard bytes; a second
    call; and the device's inflate over the device's output."""
    eng = H.get_engine()
    name, text, off = K.cases()[index]
    for lv in (0, 1):
        want, woff = twin[(name, lv)]
        ref, roff, sizes = K.compress(text, off, lv)
        assert want == ref and woff == roff, (name, lv)                   # (the twin is the rule)
        got = eng.bgzf_deflate(text, off, level=lv)
        data = got["data"].tobytes()
        assert list(got["status"]) == [0, -1, len(want), len(sizes)], (name, lv)
        assert data == want and list(got["piece_out_off"]) == woff and got["guard_intact"], (name, lv)
        again = eng.bgzf_deflate(text, off, level=lv)
        assert again["data"].tobytes() == data and list(again["status"]) == list(got["status"])
        if not data:
            continue
        blk = np.array([a for a, _, _, _ in K.parse_blocks(data)], dtype=np.int64)
        back = eng.bgzf_inflate(data, blk)
        assert list(back["status"]) == [0, -1, len(text), 0] and back["guard_intact"]
        assert back["data"].tobytes() == text, (name, lv)


def test_too_little_room_is_an_overflow_that_names_the_size():
    eng = H.get_engine()
    by = {name: (text, off) for name, text, off in K.cases()}
    for name in ("the golden processes' record lines", "0xff00 + 1 bytes", "1, 3 and 4 bytes"):
        text, off = by[name]
        want, woff, sizes = K.compress(text, off, 1)
        for cap in sorted({c for c in (0, woff[1] - 1, woff[len(woff) // 2], len(want) - 1) if 0 <= c < len(want)}):
            got = eng.bgzf_deflate(text, off, level=1, cap_bytes=cap, check=False)
            first = next(i for i in range(len(woff) - 1) if woff[i + 1] > cap)
            assert list(got["status"]) == [-8, first, len(want), len(sizes)], (name, cap)
            assert got["guard_intact"] and len(got["data"]) == 0             # (no payload byte, no zeroed slack: nothing was written)
            assert list(got["piece_out_off"]) == [min(x, cap) for x in woff]
        got = eng.bgzf_deflate(text, off, level=1, cap_bytes=int(got["status"][2]))
        assert got["data"].tobytes() == want and got["guard_intact"] and list(got["status"]) == [0, -1, len(want), len(sizes)]
    with pytest.raises(Exception) as e:
        eng.bgzf_deflate(by["1, 3 and 4 bytes"][0], by["1, 3 and 4 bytes"][1], cap_bytes=10)
    assert getattr(e.value, "code", None) == -8


def test_refused_arguments_and_offsets():
    eng = H.get_engine()
    text = b"chr20\t100\t.\tA\tG\n" * 10
    with pytest.raises(Exception) as e:
        eng.bgzf_deflate(text, [0, len(text)], level=2)
    assert getattr(e.value, "code", None) == -1
    for off in ([1, len(text)], [0, 50, 40, len(text)], [0, len(text) + 1], [-1, len(text)]):
        got = eng.bgzf_deflate(text, off, check=False)
        assert list(got["status"]) == [-9, -1, 0, 0] and got["guard_intact"] and not got["piece_out_off"].any(), off


def _four_regions():
    regs = [synth.config4_region_arrays(i, region_len=4000, n_samples=1, read_len=100) for i in range(4)]
    return [F.region_from_arrays(r) for r in regs]


def test_compress_text_of_a_synthetic_call():
    nc = F.NativeCaller(0, 2, 2)
    try:
        rr = _four_regions()
        opts = default_options(rlen=100)
        opts.originalMaxHaplotypes = opts.maxHaplotypes
        text = nc.call_regions(rr, ["S1"], opts).encode("ascii")
        lens = nc.region_text_lengths(4)
        assert len(text) > 1000 and int(lens.sum()) == len(text)
        z, zl = nc.compress_text(text, lens)
        with _HostDeflate():
            hz, hzl = nc.compress_text(text, lens)
        z = bytes(z)
        assert z == bytes(hz) and list(zl) == list(hzl) and int(zl.sum()) == len(z) - 28
        assert gzip.decompress(z) == text and z.endswith(K.EOF_BLOCK) and len(z) < len(text)
        want, woff, _ = K.compress(text, [0] + [int(x) for x in np.cumsum(lens)], 1)
        assert z == want + K.EOF_BLOCK
        z0, _ = nc.compress_text(text, lens, level=0, eof=False)
        assert gzip.decompress(bytes(z0)) == text and len(z0) > len(text)
    finally:
        nc.close()


def test_cli_writes_a_gz_output_gzip_reads(tmp_path):
    """`callVariants --synthetic config4:4 --output x.vcf.gz` is the header plus the records of the plain run, as BGZF with its EOF block."""
    from platypus_amd.__main__ import call_variants
    plain, packed = tmp_path / "x.vcf", tmp_path / "x.vcf.gz"
    base = ["--synthetic", "config4:4", "--bufferSize", "4000"]
    call_variants(base + ["--output", str(plain)])
    call_variants(base + ["--output", str(packed)])
    raw = packed.read_bytes()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and raw.endswith(K.EOF_BLOCK)
    blocks = K.parse_blocks(raw)
    assert len(blocks) >= 3 and blocks[-1][2] == 0
    with gzip.open(str(packed), "rt") as f:
        got = f.read()
    want = plain.read_text()
    body = lambda t: [ln for ln in t.split("\n") if not ln.startswith("##platypusOptions")]     # (the header carries the output path)
    assert body(got) == body(want) and got.startswith("##fileformat=VCFv4.0\n")
    assert sum(1 for ln in got.split("\n") if ln and not ln.startswith("#")) > 10
    # the header is a piece of its own: the records begin on a block boundary
    head = got[:got.index("#CHROM")] + got[got.index("#CHROM"):].split("\n")[0] + "\n"
    assert blocks[0][2] == len(head.encode())
