"""CPU test of the block list every host entry point for BGZF bytes shares (platypus_amd/csrc/host/bgzf_blocks.hpp): the header alone in a
stand-alone program (tests/bgzf_blocks_driver.cpp) under AddressSanitizer and UBSan where they link, on one three-block stream cut, flipped
and spliced every way its headers and trailers allow, against a plain-Python walk of the same bytes: the return code, the whole message,
the tables of the call, and what the host inflate makes of the blocks.  No case may make the program abort."""
import os
import struct
import subprocess
import zlib

import pytest

from platypus_amd import synth
from tests import bgzf_cases as B
from tests import tabix_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, BAD_INPUT = -1, -9
TEXT = b"".join(b"20\t%d\trs%d\tA\tC\t50\tPASS\tDP=%d\tGT\t0/1\n" % (1000 + 7 * k, k, k % 13) for k in range(24))
PAYLOAD = 300
STREAM = synth.bgzf_stream(TEXT, PAYLOAD, eof=False)[0]
NO_INFLATE = " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)"


def header(data, at):
    """(the block's length, ISIZE) for a valid header at data[at] whose block stays inside data, else None: the rules of
    include/platypus_mi355x.h, restated as tests/bgzf_cases.py::reference_verdict restates them."""
    n = len(data)
    if at > n - 26 or data[at:at + 4] != b"\x1f\x8b\x08\x04":
        return None
    xlen, = struct.unpack_from("<H", data, at + 10)
    if at + 12 + xlen + 8 > n:
        return None
    x, bsize = 0, None
    while x + 4 <= xlen:
        slen, = struct.unpack_from("<H", data, at + 14 + x)
        if x + 4 + slen > xlen:
            return None
        if data[at + 12 + x:at + 14 + x] == b"BC" and slen == 2 and bsize is None:
            bsize, = struct.unpack_from("<H", data, at + 16 + x)
        x += 4 + slen
    if x != xlen or bsize is None or bsize + 1 < 12 + xlen + 8 or at + bsize + 1 > n:
        return None
    isize, = struct.unpack_from("<I", data, at + bsize + 1 - 4)
    return None if isize > 65536 else (bsize + 1, isize)


def expected(data, first_u, end_c, end_u, refuse_empty):
    """What the driver prints for one case, as a dict: {"rc", "message"} and for rc 0 the tables and the inflate's verdict."""
    if not (0 <= first_u <= 65535 and 0 <= end_u <= 65536 and -1 <= end_c <= len(data)):
        return {"rc": INVALID, "message": ""}
    blocks, at = [], 0
    while at < len(data):
        h = header(data, at)
        if h is None:
            return {"rc": BAD_INPUT, "message": "driver: the BGZF blocks of chunk 0 do not chain: no valid block header at offset %d of its data "
                                                 "(bad magic, no BC subfield, or a block that leaves the data)" % at}
        blocks.append((at, h[0], h[1]))
        at += h[0]
    assert not blocks or blocks == T.blocks_of(data)
    sizes = [isize for _, _, isize in blocks]
    empty = [b for b, isize in enumerate(sizes) if isize == 0 and any(sizes[b:])]
    if refuse_empty and empty:
        return {"rc": BAD_INPUT, "message": "driver: block %d of chunk 0 is empty (ISIZE 0) with data behind it: tabix ends a fetch, or cuts a line, there" % empty[0]}
    to_end = end_c < 0 or (end_c == len(data) and end_u == 0)
    starts = [a for a, _, _ in blocks]
    if not to_end and end_c not in starts:
        return {"rc": BAD_INPUT, "message": "driver: end_coffset %d of chunk 0 is not a block boundary of its data" % end_c}
    inflated = [sum(sizes[:b]) for b in range(len(blocks))]
    total = sum(sizes)
    stop_blk = -1 if to_end else starts.index(end_c)
    stop = total if to_end else min(inflated[stop_blk] + end_u, total)
    out = {"rc": 0, "message": "", "chunk": [0, len(blocks), first_u, stop_blk, 0 if to_end else end_u, len(data), total], "off": starts,
           "limit": [len(data)] * len(blocks), "inflated": inflated, "span": [first_u, stop, total], "inflate": -1, "refused": "", "data": b""}
    for b, (a, n, _) in enumerate(blocks):
        payload = B.reference_verdict(data[a:a + n])
        if payload is None:
            out.update(inflate=b, refused="driver: block %d of chunk 0" % b + NO_INFLATE, data=None)
            break
        out["data"] += payload
    return out


def cases():
    """[(data, first_uoffset, end_coffset, end_uoffset)], each run with and without the refusal of empty blocks."""
    blocks = T.blocks_of(STREAM)
    assert len(blocks) == 3 and all(n > 100 for _, n, _ in blocks) and [isize for _, _, isize in blocks] == [300, 300, len(TEXT) - 600]
    out = [(STREAM[:n], 0, -1, 0) for n in range(len(STREAM) + 1)]                                        # every prefix (the first: no data at all)
    for at, n, _ in blocks:
        for byte in list(range(at, at + 18)) + list(range(at + n - 8, at + n)):
            out += [(STREAM[:byte] + bytes([STREAM[byte] ^ 1 << bit]) + STREAM[byte + 1:], 0, -1, 0) for bit in range(8)]
    for at in [a for a, _, _ in blocks] + [len(STREAM)]:
        out.append((STREAM[:at] + synth.BGZF_EOF + STREAM[at:], 0, -1, 0))
    for end_u in (0, 65536):
        for end_c in [a for a, _, _ in blocks] + [a + 1 for a, _, _ in blocks] + [len(STREAM), -1]:
            out.append((STREAM, 17, end_c, end_u))
    out += [(b"", 0, 0, 0), (STREAM, 0, len(STREAM) + 1, 0), (STREAM, 65536, -1, 0), (STREAM, 0, -1, 65537), (STREAM, -1, -1, 0), (STREAM, 0, -2, 0)]
    return [c + (flag,) for c in out for flag in (0, 1)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """The driver's answers to cases(), parsed: a list of dicts as expected() makes them."""
    d = tmp_path_factory.mktemp("bgzf_blocks")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_blocks_driver.cpp"),
            "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    fin = str(d / "cases.in")
    with open(fin, "wb") as f:
        cs = cases()
        f.write(struct.pack("<I", len(cs)))
        for data, first_u, end_c, end_u, flag in cs:
            f.write(struct.pack("<I", len(data)) + data + struct.pack("<iqiI", first_u, end_c, end_u, flag))
    r = subprocess.run([exe, fin], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])           # a sanitizer report or an abort
    lines = r.stdout.split("\n")
    out, at = [], 0
    ints = lambda line, name: [int(x) for x in line.split(" ")[1:]] if line.split(" ")[0] == name else None
    for k in range(len(cs)):
        head = lines[at].split(" ")
        assert head[:2] == ["case", str(k)] and head[2] == "rc", lines[at]
        got = {"rc": int(head[3]), "message": lines[at + 1]}
        at += 2
        if got["rc"] == 0:
            for name in ("chunk", "off", "limit", "inflated", "span"):
                got[name] = ints(lines[at], name)
                at += 1
            got["inflate"], = ints(lines[at], "inflate")
            got["refused"] = lines[at + 1]
            at += 2
            got["data"] = None
            if got["inflate"] < 0:
                assert lines[at].startswith("data ")
                got["data"] = bytes.fromhex(lines[at][5:])
                at += 1
        out.append(got)
    assert lines[at:] == [""]
    return out


def test_the_walk_and_the_host_inflate_answer_as_the_python_walk(answers):
    cs = cases()
    assert len(answers) == len(cs)
    for k, (c, got) in enumerate(zip(cs, answers)):
        assert got == expected(*c), (k, c[1:], len(c[0]))


def test_the_cases_reach_every_refusal_and_every_table(answers):
    """Each refusal of the walk and of the inflate occurs, flips included that leave the chain whole; the whole stream inflates to its text."""
    said = lambda word: sum(word in a["message"] for a in answers)
    # (an EOF block in front of each of three blocks, refused when asked to; a byte past each of three starts at both end_uoffsets and
    #  data_len with end_uoffset 65536, with and without the flag)
    assert said("do not chain") > 500 and said("is empty") == 3 and said("not a block boundary") == 2 * (2 * 3 + 1)
    assert sum(a["rc"] == INVALID for a in answers) == 10
    ok = [a for a in answers if a["rc"] == 0]
    assert sum(a["inflate"] >= 0 for a in ok) > 100 and {a["inflate"] for a in ok} == {-1, 0, 1, 2}
    assert sum(a["data"] == TEXT for a in ok) > 20 and any(a["chunk"][1] == 4 for a in ok) and any(a["chunk"][3] == 2 and a["chunk"][4] == 65536 for a in ok)
    assert zlib.crc32(TEXT) == struct.unpack_from("<I", synth.bgzf_stream(TEXT, 65536, eof=False)[0][-8:])[0]
