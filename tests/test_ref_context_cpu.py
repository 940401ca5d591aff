"""The reference context a Variant of device stage B carries (platypus_amd/csrc/host/variants.hpp, RefContext): the bytes of
[max(0, refPos - 20), min(len - 1, refPos + 21)) copied when the variant is made, read by homopolymerLengthForOneVariant, getSequenceContext and
the SNP branch of refAndAlt in place of the reference.  For every case the readers on the context give what the same readers give on the reference
itself -- value or exception -- and both give what a restatement of chaplotype.pyx:462-506 / fastafile.pyx:120-207 in Python gives; through the
debug export of libplat_caller.so, and through tests/ref_context_driver.cpp, a stand-alone program under AddressSanitizer and UBSan whose
references are heap blocks of exactly their length.  VarInfo::setPP takes float(PP) and int(float(PP)) from the integer its text is written from:
the same numbers as parsing the text."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAISES = "!Cannot have beginPos > endPos in getSequence"
POSTERIORS = [0.0, 0.49, 0.5, 1.5, 2.5, 99.5, 2500.0, 2500.5, 1e9]


def _contig(n, seed, alphabet="ACGT"):
    rng = random.Random(seed)
    s = []
    while len(s) < n:                                                   # runs of 1..6 equal bases: homopolymers on both sides of most positions
        s.extend(rng.choice(alphabet) * rng.randint(1, 6))
    return "".join(s[:n])


def _cases():
    """(reference, pos, remPos, nRemoved, added).  Contigs of 20, 41, 42 and 300 bases and one with lower-case and N bases; every refPos in 0..25 and
    in the last 26 positions; SNP, MNP of 2 and 3, insertion, deletions of 1, 19, 20 and 21 bases (19 is the longest whose removed bases the context
    always holds).  A variant with removed bases is a case only where those bases exist; an insertion also where the reference refuses the interval."""
    contigs = [_contig(20, 1), _contig(41, 2), _contig(42, 3), _contig(300, 4), _contig(300, 5, "ACGTacgtNn"), "A"]
    kinds = [("snp", 0, 1, "T"), ("mnp2", 0, 2, "TG"), ("mnp3", 0, 3, "TGA"), ("ins", 0, 0, "AC"),
             ("del1", 1, 1, ""), ("del19", 1, 19, ""), ("del20", 1, 20, ""), ("del21", 1, 21, "")]
    out = []
    for ref in contigs:
        n = len(ref)
        positions = sorted(set(range(0, 26)) | set(range(max(0, n - 26), n)) | {n, n + 5, n + 19, n + 20, n + 21, n + 30})
        for pos in positions:
            for _, shift, nrem, added in kinds:
                if nrem and pos + shift + nrem > n:
                    continue
                out.append((ref, pos, pos + shift, nrem, added))
    return out


def _get_sequence(ref, b, e):                                            # fastafile.pyx:173-207
    b, e = max(0, b), min(len(ref) - 1, e)
    if e < b:
        raise IndexError
    return ref[b:e]


def _model(ref, pos, rem_pos, nrem, added):
    """HP, SC, REF of the record at refPos, removed bases -- the fields of probeRefContext behind CTX."""
    def guarded(f):
        try:
            return f()
        except IndexError:
            return RAISES

    def hp():
        left, right = _get_sequence(ref, pos - 20, pos), _get_sequence(ref, pos + 1, pos + 21)
        if not left or not right:
            return "0"
        nl, nr = len(left) - len(left.rstrip(left[-1])), len(right) - len(right.lstrip(right[0]))
        return str(max(nl, nr) if left[-1] != right[0] else nl + nr)

    def refalt():
        if nrem == 1 and len(added) == 1:
            return "-" if pos >= len(ref) else ref[pos]                  # getCharacter
        return _get_sequence(ref, pos, pos + nrem + (1 if nrem != len(added) else 0))

    return "HP=%s\tSC=%s\tREF=%s\tREM=%s" % (guarded(hp), guarded(lambda: _get_sequence(ref, pos - 10, pos + 11)), guarded(refalt), ref[rem_pos:rem_pos + nrem])


def _has_context(ref, pos):
    return min(len(ref) - 1, pos + 21) >= max(0, pos - 20)


@pytest.fixture(scope="module")
def native():
    from platypus_amd import fastcaller as F
    F.build()
    lib = C.CDLL(F.LIB_PATH)
    lib.plat_caller_debug_ref_context.restype = None
    lib.plat_caller_debug_ref_context.argtypes = [C.c_char_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    lib.plat_caller_debug_set_pp.restype = None
    lib.plat_caller_debug_set_pp.argtypes = [C.c_double, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    return lib


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_the_cases_hold_what_they_should(cases):
    refs = {c[0] for c in cases}
    assert sorted(len(r) for r in refs) == [1, 20, 41, 42, 300, 300] and any("n" in r and "N" in r and "a" in r for r in refs)
    for ref in refs:
        mine = [c for c in cases if c[0] is ref or c[0] == ref]
        assert {c[3] for c in mine if c[1] == 0} >= ({0, 1, 2, 3, 19} if len(ref) >= 20 else {0, 1})
        assert {c[1] for c in mine} >= set(range(0, 26)) | set(range(max(0, len(ref) - 26), len(ref)))
    # both sides of the boundary of the removed bases: 19 always inside the context, 21 never, 20 inside unless the contig's end clamps it
    assert any(c[3] == 19 for c in cases) and any(c[3] == 20 for c in cases) and any(c[3] == 21 for c in cases)
    # the two ways getSequence raises: HP's right flank at the contig's last base (the context exists), and the whole interval behind the contig (no context)
    assert any(c[1] == len(c[0]) - 1 and _has_context(c[0], c[1]) and RAISES in _model(*c) for c in cases)
    assert any(not _has_context(c[0], c[1]) and _model(*c).count(RAISES) >= 2 for c in cases)


def test_context_and_reference_give_the_same(native, cases):
    buf = C.create_string_buffer(512)
    n_ctx = 0
    for ref, pos, rem_pos, nrem, added in cases:
        got = []
        for with_context in (0, 1):
            native.plat_caller_debug_ref_context(ref.encode(), len(ref), pos, rem_pos, nrem, added.encode(), with_context, buf, 512)
            got.append(buf.value.decode())
        want = _model(ref, pos, rem_pos, nrem, added)
        assert got[0] == "CTX=0\t" + want, (ref, pos, rem_pos, nrem, added)
        assert got[1] == "CTX=%d\t" % _has_context(ref, pos) + want, (ref, pos, rem_pos, nrem, added)
        n_ctx += _has_context(ref, pos)
    assert n_ctx > len(cases) // 2


def test_stand_alone_program_under_sanitizers(tmp_path, cases):
    exe = str(tmp_path / "ref_context_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I", os.path.join(ROOT, "platypus_amd", "csrc"), os.path.join(ROOT, "tests", "ref_context_driver.cpp"), "-o", exe])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for ref, pos, rem_pos, nrem, added in cases:
            f.write("%s %d %d %d %s\n" % (ref, pos, rem_pos, nrem, added or "-"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (as tests/test_bgzf_cpu.py: a library loaded in front of ASan's runtime is no error)
    out = subprocess.run([exe, path], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 2 * len(cases) + len(POSTERIORS) + 5
    for k, c in enumerate(cases):
        want = _model(*c)
        assert lines[2 * k] == "CTX=0\t" + want and lines[2 * k + 1] == "CTX=%d\t" % _has_context(c[0], c[1]) + want, c
    for line, p in zip(lines[2 * len(cases):], POSTERIORS):
        head, parsed = line.split(" | ")
        assert head.split(": ")[1].split(" ")[1:] == parsed.split(" ") and head.split(": ")[1].split(" ")[0] == "%.0f" % p, line
    assert lines[-5:] == ["NO_REFCTX unset: noRefCtx=0", "NO_REFCTX empty: noRefCtx=0", "NO_REFCTX 0: noRefCtx=0", "NO_REFCTX 1: noRefCtx=1", "NO_REFCTX yes: noRefCtx=0"]


@pytest.mark.parametrize("posterior", POSTERIORS)
def test_set_pp_gives_the_numbers_of_its_text(native, posterior):
    got = []
    for via_text in (0, 1):
        pp, num, integer = C.create_string_buffer(64), C.c_double(), C.c_int()
        native.plat_caller_debug_set_pp(posterior, via_text, pp, 64, C.byref(num), C.byref(integer))
        got.append((pp.value.decode(), num.value, integer.value))
    text = "%.0f" % posterior                                            # ties to even on the exact value, as C's printf
    assert got[0] == got[1] == (text, float(text), int(float(text)))
