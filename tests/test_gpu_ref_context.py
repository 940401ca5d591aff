"""The reference context of device stage B's variants (RefContext, platypus_amd/csrc/host/variants.hpp) in the region loop: three hand-made
one-sample regions whose variants lie where the context is clamped, or is not used -- SNPs 3 bases from either end of a 300-base contig and in its
middle; a 1-base deletion and an insertion next to the ends of the same contig; a 25-base deletion (its removed bases are longer than the
context) in a 2 000-base region.  The record text of the default run is byte for byte the text with PLAT_CALLER_NO_REFCTX=1 (HP, SC and REF read
from the reference, as before the context existed) and with PLAT_CALLER_HOST_B=1 (the host's own stage B, whose variants never carry one; its
HP / SC are pinned by the region goldens).  The SNP at 296 becomes a Variant with a context clamped at the contig's end but no record: every
100-base read that covers it ends within three bases of the haplotype's end, and reads that end so close to it support no call (a SNP at 285 in
reads ending at 292 to 294 is not called either), with any of the three settings.
Fourteen more reads that end at 286 to 288 carry a SNP at 281: its context is clamped at the contig's end too ([261, 299)), it is called, and its
record's REF, HP and SC are read through that context; so is the SC (19 bases) of the insertion at 290.  The three runs share the pytest
process, as the runs of tests/test_gpu_packed_direct.py do: the switches are read at every call, which is all that sharing it relies on."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("PLAT_CALLER_NO_REFCTX", "PLAT_CALLER_HOST_B")
READ_LEN = 100


def _contig(n, seed):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def _other(b):
    return b"ACGT"[(b"ACGT".index(b) + 1) % 4]


def _read(ref, pos, snps=(), deletion=None, insertion=None, k=0):
    """A read of READ_LEN bases from `pos` that follows `ref` but for SNPs at the given positions, a deletion (refPos, length: the bases behind
    refPos are missing) or an insertion (refPos, bases: they follow the base at refPos), with the CIGAR an aligner would report."""
    from platypus_amd import hostapi as H
    if deletion:
        p, d = deletion
        a = p + 1 - pos
        seq = ref[pos:p + 1] + ref[p + 1 + d:p + 1 + d + READ_LEN - a]
        cigar, end = [(0, a), (2, d), (0, READ_LEN - a)], pos + READ_LEN + d
    elif insertion:
        p, ins = insertion
        a = p + 1 - pos
        seq = ref[pos:p + 1] + ins + ref[p + 1:p + 1 + READ_LEN - a - len(ins)]
        cigar, end = [(0, a), (1, len(ins)), (0, READ_LEN - a - len(ins))], pos + READ_LEN - len(ins)
    else:
        seq, cigar, end = ref[pos:pos + READ_LEN], [(0, READ_LEN)], pos + READ_LEN
    seq = bytearray(seq)
    for s in snps:
        if pos <= s < pos + READ_LEN:
            seq[s - pos] = _other(ref[s])
    assert len(seq) == READ_LEN and end <= len(ref) - 1
    return H.AlignedRead(bytes(seq), bytes([35]) * READ_LEN, pos, 60, 16 if k % 2 else 0, end=end, cigarOps=cigar)


def _inputs():
    """(fasta, [(chrom, start, end, [bamReadBuffer])], expected record lines per contig)."""
    from platypus_amd import hostapi as H
    small, big = _contig(300, 3101), _contig(2400, 3102)
    refs = {"snps": small, "indels": small, "longdel": big}
    reads = {
        # 58 reads: SNPs at 3, 150 and 296 (the contig's last readable base is 298), and one at 281 in reads that end before 290
        "snps": [_read(small, 1 + k % 3, snps=(3,), k=k) for k in range(14)] + [_read(small, 60 + 4 * k, snps=(150,), k=k) for k in range(16)] +
                [_read(small, 197 + k % 3, snps=(296,), k=k) for k in range(14)] + [_read(small, 186 + k % 3, snps=(281,), k=k) for k in range(14)],
        # 56 reads: a 1-base deletion behind position 5, an insertion behind position 290
        "indels": [_read(small, 1 + k % 3, deletion=(5, 1), k=k) for k in range(18)] + [_read(small, 60 + 4 * k, k=k) for k in range(20)] +
                  [_read(small, 197 + k % 3, insertion=(290, b"TG" if small[291:293] != b"TG" else b"CA"), k=k) for k in range(18)],
        # 48 reads: a 25-base deletion behind position 1000
        "longdel": [_read(big, 920 + 3 * k % 70, deletion=(1000, 25), k=k) for k in range(48)],
    }
    fasta = H.FastaFile(refs)
    work = []
    for chrom, (s, e) in (("snps", (0, 300)), ("indels", (0, 300)), ("longdel", (200, 2200))):
        rs = sorted(reads[chrom], key=lambda a: a.pos)
        assert 40 <= len(rs) <= 60
        work.append((chrom, s, e, [H.bamReadBuffer(rs, [], [], sample="S1")]))
    return fasta, work, {"snps": 3, "indels": 2, "longdel": 1}


def _run(fasta, work, switch=None):
    """Record text and counters of one call over the three regions (one chunk), `switch` set to 1 in the environment and the other unset."""
    from platypus_amd import fastcaller as F
    from platypus_amd.options import default_options
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    if switch:
        os.environ[switch] = "1"
    try:
        o = default_options()
        o.minFlank = 0                                                       # (the variants 3 bases from a read's end are candidates at all)
        rs = [F.RegionReads.from_buffers(c, s, e, fasta, b, packed=True) for c, s, e, b in work]
        nc = F.NativeCaller(0, 1, 4)
        try:
            txt = nc.call_regions(rs, ["S1"], o)
            return bytes(txt) if not isinstance(txt, (bytes, str)) else txt, dict(nc.stats)
        finally:
            nc.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_record_text_is_the_same_with_and_without_the_reference_context():
    fasta, work, expected = _inputs()
    here, st = _run(fasta, work)
    print(here if isinstance(here, str) else here.decode())
    plain, st_plain = _run(fasta, work, "PLAT_CALLER_NO_REFCTX")
    host, st_host = _run(fasta, work, "PLAT_CALLER_HOST_B")
    again, _ = _run(fasta, work)
    # the default run took the context's path for every region, the third none
    assert st["n_regions_stage_b_device"] == 3 and st["n_regions_stage_b_host"] == 0
    assert st_plain["n_regions_stage_b_device"] == 3 and st_host["n_regions_stage_b_device"] == 0
    text = here if isinstance(here, str) else here.decode()
    lines = [x.split("\t") for x in text.splitlines() if x and not x.startswith("#")]
    for chrom, n in expected.items():
        assert sum(x[0] == chrom for x in lines) == n, (chrom, text)
    assert {(x[0], int(x[1])) for x in lines} >= {("snps", 4), ("snps", 151), ("snps", 282), ("indels", 6), ("indels", 291)}
    assert st["n_variants"] == st_plain["n_variants"] == st_host["n_variants"] == 7       # (the SNP at 296 among them)
    small = fasta._seq["snps"]
    right = [x for x in lines if x[0] == "snps" and int(x[1]) == 282]
    assert len(right) == 1 and right[0][3] == small[281:282].decode() and "SC=" + small[271:292].decode() + ";" in right[0][7]
    assert any(x[0] == "indels" and "SC=" + fasta._seq["indels"][280:299].decode() + ";" in x[7] for x in lines)
    assert any(x[0] == "longdel" and len(x[3]) == 26 and len(x[4]) == 1 for x in lines)
    assert all("HP=" in x[7] and "SC=" in x[7] for x in lines)
    assert here == plain
    assert here == host
    assert here == again
