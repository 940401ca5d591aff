"""GPU tests of the front of the fetched, BAM and BGZF region loops against the oracle, off the shapes of tests/golden/readqc_cases.json.gz:
checkAndTrimRead in its three storages (plat_read_qc_batch, plat_read_buffers_batch, plat_read_buffers_packed_batch: k_read_qc and
k_read_qc_packed over QualBytes, QualPacked and QualPackedPlain) and the split of every stream into its two read buffers (k_read_split,
k_read_gather), on the inputs of tests/read_qc_cases.py.  What the buffers must hold is built in numpy from the ORACLE's verdicts; every
comparison is of integers and bytes and is exact.  tests/test_read_qc_cases_cpu.py shows what the inputs reach."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from platypus_amd import _lib, hostapi as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_qc_cases as Q  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("qc", "ascii", "packed")


def pack(tab):
    """A table's bases and qualities as PLAT_READS_PACKED bytes with their exceptions (bases other than A/C/G/T, qualities above 63).  The
    quality bits of an exception's byte are unspecified: 63 for a quality above 63, and for another letter with quality 1..63 a value that
    is NOT its quality (63 - q), so that a kernel reading the byte instead of the exception is seen."""
    seq, qual = tab["seq"], tab["qual"]
    is_exc = ~np.isin(seq, Q.ACGT) | (qual > 63)
    bits = np.where(is_exc & (qual <= 63), np.where(qual == 0, 0, 63 - qual.astype(np.int32)), np.minimum(qual, 63)).astype(np.uint8)
    exc = np.nonzero(is_exc)[0].astype(np.int64)
    return dict(packed=(((seq >> 1) & 3) | (bits << 2)).astype(np.uint8), exc_index=exc, exc_base=seq[exc].copy(), exc_qual=qual[exc].copy())


def run_device(tab, opt, mode, tables=True, pk=None):
    """One call of plat_read_qc_batch ('qc'), plat_read_buffers_batch ('ascii') or plat_read_buffers_packed_batch ('packed') on a table.
    Every device array has at least one entry more than the call may touch."""
    import torch
    eng = H.get_engine()
    n, ns = len(tab["pos"]), len(tab["sbeg"]) - 1
    nb, npairs = int(tab["off"][-1]), int(tab["coff"][-1])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    more = lambda a, k=1: np.concatenate([a, np.zeros(k, dtype=a.dtype)])
    sof = np.repeat(np.arange(ns, dtype=np.int32), np.diff(tab["sbeg"]))
    d = dict(off=dev(tab["off"], np.int64), pos=dev(more(tab["pos"]), np.int32), end=dev(more(tab["end"]), np.int32), mapq=dev(more(tab["mapq"]), np.uint8),
             flags=dev(more(tab["flags"]), np.int32), cid=dev(more(tab["cid"]), np.int16), mcid=dev(more(tab["mcid"]), np.int16),
             ins=dev(more(tab["ins"]), np.int32), mpos=dev(more(tab["mpos"]), np.int32), cig=dev(more(tab["cig"], 2), np.int16),
             coff=dev(tab["coff"], np.int32), sof=dev(more(sof), np.int32), sbeg=dev(tab["sbeg"], np.int32))
    if mode == "packed":
        pk = pk or pack(tab)
        ne = len(pk["exc_index"])
        d["blob"] = dev(more(pk["packed"], _lib.PLAT_BLOB_PAD), np.uint8)
        if ne:
            d.update(ei=dev(pk["exc_index"], np.int64), eb=dev(pk["exc_base"], np.uint8), eq=dev(pk["exc_qual"], np.uint8))
        b = _lib.ReadBuffersPackedIn()
    else:
        d["qual"] = dev(more(tab["qual"], _lib.PLAT_BLOB_PAD), np.uint8)
        d["blob"] = dev(more(tab["seq"], _lib.PLAT_BLOB_PAD), np.uint8)
        b = _lib.ReadBuffersIn()
    q = b.qc
    q.n_reads = n
    q.read_qual, q.read_off, q.read_pos, q.read_mapq, q.read_flags = (0 if mode == "packed" else d["qual"].data_ptr()), d["off"].data_ptr(), d["pos"].data_ptr(), d["mapq"].data_ptr(), d["flags"].data_ptr()
    q.chrom_id, q.mate_chrom_id, q.insert_size, q.mate_pos = d["cid"].data_ptr(), d["mcid"].data_ptr(), d["ins"].data_ptr(), d["mpos"].data_ptr()
    q.cigar, q.cig_off, q.stream_of = d["cig"].data_ptr(), d["coff"].data_ptr(), d["sof"].data_ptr()
    b.n_streams, b.stream_begin, b.read_end = ns, d["sbeg"].data_ptr(), d["end"].data_ptr()
    if mode == "packed":
        b.read_packed = d["blob"].data_ptr()
        b.n_exc = ne
        b.exc_index, b.exc_base, b.exc_qual = (d["ei"].data_ptr(), d["eb"].data_ptr(), d["eq"].data_ptr()) if ne else (None, None, None)   # NULL without exceptions
    else:
        b.read_seq = d["blob"].data_ptr()
    o = _lib.ReadQCOptions(opt["minGoodQualBases"], opt["minMapQual"], opt["minBaseQual"], opt["trimOverlapping"], opt["trimAdapter"],
                           opt["trimReadFlank"], opt["trimSoftClipped"], *[int(x) for x in opt["enabled"]])
    fill = lambda k, dt, v: torch.full((k + 1,), v, dtype=dt, device=eng.device)
    ok, why, perm, counts = fill(n, torch.int32, -7), fill(n, torch.int32, -7), fill(n, torch.int32, -7), fill(10 * ns, torch.int32, -7)
    g = dict(off=fill(n + 2 * ns, torch.int64, -7), cig_off=fill(n + 2 * ns, torch.int32, -7), seq=fill(nb + _lib.PLAT_BLOB_PAD, torch.uint8, 0xEE),
             qual=None if mode == "packed" else fill(nb + _lib.PLAT_BLOB_PAD, torch.uint8, 0xEE), cigar=fill(2 * npairs + 1, torch.int16, -7),
             pos=fill(n, torch.int32, -7), end=fill(n, torch.int32, -7), mapq=fill(n, torch.uint8, 0xEE), flags=fill(n, torch.int32, -7),
             mate_pos=fill(n, torch.int32, -7))
    if mode == "qc":
        rc = eng.lib.plat_read_qc_batch(eng.ctx, C.byref(q), C.byref(o), ok.data_ptr(), why.data_ptr(), eng._stream())
    else:
        t = _lib.ReadBuffersTables(*[(g[k].data_ptr() if g[k] is not None else 0) for k, _ in _lib.ReadBuffersTables._fields_])
        fn = eng.lib.plat_read_buffers_packed_batch if mode == "packed" else eng.lib.plat_read_buffers_batch
        rc = fn(eng.ctx, C.byref(b), C.byref(o), ok.data_ptr(), why.data_ptr(), perm.data_ptr(), counts.data_ptr(), C.byref(t) if tables else None,
                eng._stream())
    _lib.check(rc, "read QC (%s)" % mode)
    eng._sync()
    h = lambda x: x.cpu().numpy()
    out = dict(ok=h(ok)[:n], reason=h(why)[:n], flags=h(d["flags"])[:n], perm=h(perm)[:n], counts=h(counts)[:10 * ns])
    if mode == "packed":
        out["packed"] = h(d["blob"])[:nb]
        out["exc_qual"] = h(d["eq"]) if ne else np.zeros(0, np.uint8)
        out["pk"] = pk
    else:
        out["qual"] = h(d["qual"])[:nb]
    if mode != "qc" and tables:
        out["t"] = {k: h(v) for k, v in g.items() if v is not None}
    # nothing written behind what the call owns
    assert h(ok)[n] == -7 and h(why)[n] == -7 and h(perm)[n] == -7 and h(counts)[10 * ns] == -7
    if mode != "qc":
        assert all(h(g[k])[-1] == -7 for k in ("off", "cig_off", "cigar", "pos", "end", "flags", "mate_pos")) and (h(g["seq"])[nb:] == 0xEE).all()
    return out


def check(tab, want, out, mode, tables=True):
    """A call's outputs against the oracle's (ok, reason, flags, qual) of the table: verdicts, trimmed qualities in their storage, and, for
    the buffer calls, the split and the gathered buffers."""
    ok, why, flags, qual = want
    n, nb, npairs = len(ok), int(tab["off"][-1]), int(tab["coff"][-1])
    assert np.array_equal(out["ok"], ok) and np.array_equal(out["reason"], why) and np.array_equal(out["flags"], flags)
    if mode == "packed":
        pk = out["pk"]
        exc, before = pk["exc_index"], pk["packed"]
        # a trimmed byte keeps its base bits and gets quality bits 0; a trimmed exception's quality is 0, an untouched one's its input
        gone = (qual == 0)                                            # (a byte whose quality was 0 holds quality bits 0 already: pack())
        bytes_want = np.where(gone, before & 3, before)
        assert np.array_equal(out["packed"], bytes_want)
        assert np.array_equal(out["exc_qual"], qual[exc])
        assert np.array_equal(out["packed"] & 3, before & 3)
        decoded = (out["packed"] >> 2).astype(np.uint8)
        decoded[exc] = out["exc_qual"]
        plain = np.ones(nb, bool); plain[exc] = False
        assert np.array_equal(decoded[plain], qual[plain]) and np.array_equal(decoded[exc], qual[exc])
    else:
        assert np.array_equal(out["qual"], qual)
    if mode == "qc":
        return
    exp = Q.expected_split(tab, ok, why)
    assert np.array_equal(out["perm"], exp["perm"])
    assert np.array_equal(out["counts"], exp["counts"])
    if not tables:
        return
    t = out["t"]
    assert np.array_equal(t["off"][:-1], exp["t_off"]) and np.array_equal(t["cig_off"][:-1], exp["t_cigoff"])
    src = bytes_want if mode == "packed" else tab["seq"]
    assert np.array_equal(t["seq"][:nb], src[exp["byte_index"]])
    if mode != "packed":
        assert np.array_equal(t["qual"][:nb], qual[exp["byte_index"]])
    assert np.array_equal(t["cigar"][:2 * npairs], tab["cig"][exp["short_index"]])
    p = exp["perm"]
    assert np.array_equal(t["pos"][:n], tab["pos"][p]) and np.array_equal(t["end"][:n], tab["end"][p]) and np.array_equal(t["mapq"][:n], tab["mapq"][p])
    assert np.array_equal(t["flags"][:n], flags[p]) and np.array_equal(t["mate_pos"][:n], tab["mpos"][p])


@functools.lru_cache(maxsize=None)
def oracle_runs():
    """The oracle over every generated call, once for the module: [(call, table, (ok, reason, flags, qual))], read-only."""
    from oracle.oracle import Oracle
    orc = Oracle()
    out = []
    for c in Q.calls():
        tab = Q.table_of(c["streams"])
        out.append((c, tab, Q.oracle_table(orc, tab, c["opt"])))
    return out


# ---- every generated stream, in its multi-stream calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_verdicts_trimming_split_and_buffers_equal_the_oracle(mode):
    """Every call of tests/read_qc_cases.py (streams of 0..1025 reads in every verdict pattern, the empty streams among them) through one
    storage: ok, reason, flags and trimmed qualities read for read; for the two buffer calls also perm, counts, the offset tables and the
    gathered seq / qual / cigar / pos / end / mapq / flags / mate_pos byte for byte, built from the oracle's verdicts."""
    runs = oracle_runs()
    gathered_lengths, gathered_pairs, n = set(), set(), 0
    for c, tab, want in runs:
        check(tab, want, run_device(tab, c["opt"], mode), mode)
        gathered_lengths |= set(np.diff(tab["off"]).tolist()); gathered_pairs |= set(np.diff(tab["coff"]).tolist())
        n += len(tab["pos"])
    assert n > 20000 and {0, 641, 1000} <= gathered_lengths and {0, 33, 79} <= gathered_pairs


def test_calls_without_tables_give_the_same_verdicts_and_split():
    """plat_read_buffers_batch with tab == NULL (ranks only): ok, reason, perm and counts of the call with tables -- both held to the oracle."""
    runs = oracle_runs()
    for c, tab, want in [r for r in runs if r[0]["name"] in ("patterns0", "patterns1", "order", "fuzz3", "fuzz20")]:
        for mode in ("ascii", "packed"):
            bare, full = run_device(tab, c["opt"], mode, tables=False), run_device(tab, c["opt"], mode)
            check(tab, want, bare, mode, tables=False)
            for k in ("ok", "reason", "perm", "counts", "flags"):
                assert np.array_equal(bare[k], full[k]), k


# ---- the exception edges of the packed path -------------------------------------------------------------------------------------------------
def _read(pos, qual, seq=None, flag=0, cigar=None, ins=0):
    L = len(qual)
    return dict(seq=seq or (b"ACGT" * L)[:L], qual=bytes(qual), pos=pos, end=pos + L, mapq=60, flag=flag, chromID=1, mateChromID=1, insertSize=ins,
                matePos=pos + 200, cigar=[[0, L]] if cigar is None else cigar)


def _oracle(tab, opt):
    from oracle.oracle import Oracle
    return Q.oracle_table(Oracle(), tab, opt)


def test_packed_exceptions_at_the_edges_of_reads_and_of_the_blob():
    """Reads of 30 bases that are accepted only if all 30 count as good (minGoodQualBases 30), so that one exception seen or missed turns a
    verdict: on the blob's first and last byte, on a read's own first and last byte, on the last byte of the read before and the first byte
    of the read after a read that has none (which must see none), and an N whose quality is below the threshold while its byte's quality
    bits are above it.  Then the same edges where they are trimmed instead (minGoodQualBases 0)."""
    good = [30] * 30
    at = lambda k, v: good[:k] + [v] + good[k + 1:]
    n_seq = lambda k: (b"ACGT" * 8)[:k] + b"N" + (b"ACGT" * 8)[k + 1:30]
    reads = [_read(100, at(0, 200)),                                   # 0: the blob's first byte, a negative quality: rejected
             _read(110, at(29, 200)),                                  # 1: its own last byte: rejected
             _read(120, good),                                         # 2: none of its own, exceptions on both neighbours' nearest bytes: accepted
             _read(130, at(0, 200)),                                   # 3: its own first byte: rejected
             _read(140, at(0, 100)),                                   # 4: a good exception on its first byte: accepted
             _read(150, at(29, 127)),                                  # 5: ... on its last: accepted
             _read(160, at(5, 10), seq=n_seq(5)),                      # 6: N of quality 10 in a byte whose quality bits say 53: rejected
             _read(170, at(5, 20), seq=n_seq(5)),                      # 7: N of quality 20 (bits 43): accepted
             _read(180, good),                                         # 8
             _read(190, at(29, 200))]                                  # 9: the blob's last byte: rejected
    tab = Q.table_of([reads[:5], reads[5:]])
    opt = Q.options(minGoodQualBases=30, minBaseQual=20, minMapQual=20)
    want = _oracle(tab, opt)
    assert want[0].tolist() == [0, 0, 1, 0, 1, 1, 0, 1, 1, 0]
    pk = pack(tab)
    assert pk["exc_index"].tolist() == [0, 59, 90, 120, 179, 185, 215, 299] and (pk["packed"][[185, 215]] >> 2).tolist() == [53, 43]
    check(tab, want, run_device(tab, opt, "packed", pk=pk), "packed")
    check(tab, want, run_device(tab, opt, "ascii"), "ascii")
    # trimmed: forward reads lose their tail below 5 (a negative byte is below 5), reverse reads their head; 64..127 stays
    reads = [_read(100, at(0, 3), seq=n_seq(0), flag=16),              # the blob's first byte, an N of quality 3 (bits 60) on a reverse read: trimmed
             _read(110, good[:28] + [2, 130]),                         # its own last byte negative, the byte before it 2: both trimmed
             _read(120, good),
             _read(130, [255, 1] + good[2:], flag=16),                 # its own first byte negative on a reverse read
             _read(140, at(29, 100)),                                  # a good exception on the last byte: stays 100
             _read(150, [64] + good[1:], flag=16),
             _read(160, at(29, 4), seq=n_seq(29)),                     # an N of quality 4 (bits 59) on the last byte: trimmed
             _read(170, at(29, 5), seq=n_seq(29)),                     # ... of quality 5 (bits 58): stays
             _read(180, at(29, 128))]                                  # the blob's last byte
    tab = Q.table_of([reads[:2], [], reads[2:]])
    opt = Q.options(minGoodQualBases=0, minBaseQual=20, minMapQual=20, trimReadFlank=0)
    want = _oracle(tab, opt)
    assert want[0].all() and want[3][[0, 58, 59, 90, 91, 149, 150, 209, 239, 269]].tolist() == [0, 0, 0, 0, 0, 100, 64, 0, 5, 0]
    for mode in MODES:
        check(tab, want, run_device(tab, opt, mode), mode)


def test_packed_call_without_exceptions_and_with_min_base_qual_64():
    """n_exc == 0 with NULL exception arrays; and minBaseQual 64, where no plain byte counts as good and only exceptions of 64..127 do."""
    rng = np.random.default_rng(5)
    opt = Q.options(minGoodQualBases=28, minBaseQual=20, minMapQual=20, trimReadFlank=5)
    reads = [_read(100 + 3 * k, rng.integers(0, 64, 40).tolist(), flag=int(rng.choice([0, 16]))) for k in range(130)]
    tab = Q.table_of([reads[:70], reads[70:]])
    pk = pack(tab)
    assert len(pk["exc_index"]) == 0
    want = _oracle(tab, opt)
    assert 20 < want[0].sum() < 110
    check(tab, want, run_device(tab, opt, "packed", pk=pk), "packed")
    opt = Q.options(minGoodQualBases=3, minBaseQual=64, minMapQual=20, trimReadFlank=0)
    q63 = [63] * 20
    put = lambda vals: [vals[k // 5] if k % 5 == 2 and k // 5 < len(vals) else 63 for k in range(20)]
    reads = [_read(100, q63), _read(110, put([64, 100, 127])), _read(120, put([64, 127])), _read(130, put([64, 100, 128])),
             _read(140, put([64, 64, 64, 255])), _read(150, put([127, 200, 127]))]
    tab = Q.table_of([reads])
    want = _oracle(tab, opt)
    assert want[0].tolist() == [0, 1, 0, 0, 1, 0] and (want[1][want[0] == 0] == 0).all()
    for mode in MODES:
        check(tab, want, run_device(tab, opt, mode), mode)


# ---- past the verdict masks kept in LDS ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("ascii", "packed"))
def test_a_stream_past_262144_reads_between_two_short_ones(mode):
    """262 144 + 700 reads in one stream (the split takes the last ballots again from out_ok), a short stream before it and one behind it
    in the same call: verdicts, perm, counts, offsets (those behind the long stream start where they should) and the gathered buffers in
    full.  And the same call without tables."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(11)
    opt = Q.long_options()
    short = [Q.table_of([Q.pattern_stream(rng, n, 500, opt, set(range(0, n, 3)), "dup")]) for n in (65, 130)]
    tab = Q.concat_tables([short[0], Q.long_table(), short[1]])
    assert tab["sbeg"].tolist() == [0, 65, 65 + Q.LONG_READS, 65 + Q.LONG_READS + 130]
    want = Q.oracle_table(Oracle(), tab, opt)
    check(tab, want, run_device(tab, opt, mode), mode)
    check(tab, want, run_device(tab, opt, mode, tables=False), mode, tables=False)


# ---- the one place where the device is defined and the reference is not ----------------------------------------------------------------------
def test_a_soft_clip_longer_than_its_read_is_trimmed_to_the_reads_end_only():
    """DEVICE ONLY: no reference and no oracle answer exists for a CIGAR that claims more soft-clipped bases than the read holds (the
    reference writes behind the read's qualities).  The device trims up to the read's end, leaves the next read's first quality alone and
    accepts the read (the `index < rlen` clamp of read_qc_one; DESIGN.md, the fetched front end)."""
    good = [30] * 20
    reads = [_read(100, good), _read(110, good, cigar=[[0, 12], [4, 50]]), _read(120, [31] + good[1:]), _read(130, good, cigar=[[4, 32767]])]
    tab = Q.table_of([reads])
    opt = Q.options(minGoodQualBases=0, minBaseQual=20, minMapQual=20, trimReadFlank=0)
    for mode in MODES:
        out = run_device(tab, opt, mode)
        if mode == "packed":
            qual = (out["packed"] >> 2).astype(np.uint8)
            assert np.array_equal(out["packed"] & 3, out["pk"]["packed"] & 3)
        else:
            qual = out["qual"]
        assert out["ok"].tolist() == [1, 1, 1, 1] and out["reason"].tolist() == [-1] * 4
        assert qual[:20].tolist() == good and qual[20:40].tolist() == good[:12] + [0] * 8             # its own qualities, up to its end
        assert qual[40:60].tolist() == [31] + good[1:]                                               # the read after it: untouched
        assert qual[60:80].tolist() == [0] * 20 and len(qual) == 80
