"""What plat_stage_b_batch must write, computed on the host from the same inputs (a plain module: tests/test_stage_b_reference_cpu.py
proves it against the committed goldens, tests/test_gpu_stage_b_kernels.py compares the kernels with it).

Every step is the mirror code the goldens already pin -- regionprep.leftNormaliseIndel / filterVariants / WindowGenerator, hostapi's
ReadArray window pointers, isHaplotypeValid with itertools.combinations, Haplotype (getMutatedSequence), mergeHaplotypes, the window rules
of caller._prepareWindow, caller.order_can_matter / _py2_heap_order -- chained as callVariantsInRegion chains them.  What is NOT taken
from the mirror are the flags: which region comes back PLAT_SB_HOST with which reason code, and which window carries which PLAT_SBW_*
bit, is predicted here from the INPUTS by the rules include/platypus_mi355x.h documents for hdr[5] and PLAT_SBW_*.

One prediction is NOT independent of the kernels: PLAT_SBW_DUPLICATE.  The reference has no such notion -- the bit says what the device
chose not to decide -- so its rule (the common prefix `min(first variant's refPos, haplotype end) - lo`, the stage of 384 bytes behind
it, equal sequences with an indel or with a multi-nucleotide variant of 0 or more than 16 differences) restates the header's text, which
restates the kernel.  A kernel that computed the common prefix wrongly in the same way as _window() below would pass the flag's check;
what still catches it is the content: a window without the bit must hold mergeHaplotypes' list in sorted() order, byte for byte, and
one with the bit every valid combination, both from the mirror alone.

A region is described by a dict (region()); pack() turns a list of them into the arguments of Engine.stage_b, expected() into the
expected content, compare() asserts one against the other -- content, not placement (var_add_off may differ between runs), and the
sentinel in every element behind what a count says was written."""
import copy
import functools
import math
from itertools import combinations
from types import SimpleNamespace

import numpy as np

from platypus_amd import caller, hostapi as H
from platypus_amd.options import default_options
from platypus_amd.regionprep import WindowGenerator, filterVariants, leftNormaliseIndel
from platypus_amd.vcfrecords import py2_dict_slot_order, py2_variant_hash

PLAT_SB_HOST = 1
SBW_SKIP, SBW_HOST, SBW_DUPLICATE = 1, 2, 4
SB_CAP, SB_MAXCOMB, SB_STAGE, HASH_SIZE = 1024, 5, 384, 16384
SB_DICT_CAP = 5400                                                           # distinct records of a scan whose dictionary the device replays
SB_KEY_RUN = 48                                                              # candidates of one sort key the device looks through (more: reason 2)
ERR_OVERFLOW, ERR_BAD_INPUT = -8, -9

OPTIONS = dict(minReads=2, maxSize=1500, mergeClusteredVariants=1, maxVarDist=15, minVarDist=9, largeWindows=0, maxVariants=8, maxHaplotypes=50,
               filterVarsByCoverage=1, skipDifficultWindows=0, maxReads=5000000.0)
CAPS = dict(cap_vars=64, cap_windows=32, cap_added=256, cap_batch_windows=64, cap_batch_haps=512, cap_batch_reads=1024, cap_hap_bytes=1 << 20)


def options(**over):
    o = dict(OPTIONS)
    o.update(over)
    return o


def caps(**over):
    c = dict(CAPS)
    c.update(over)
    return c


def region(ref, cands, start=0, end=None, rlen=100, ref_seq_start=0, contig_len=None, reads=(), bad=(), broken=(), longest=None, name="20",
           merge_status=0, n_cands=None):
    """One region.  ref = contig[ref_seq_start : ref_seq_start + len(ref)]; cands = (pos, nrem, added bytes, supporting reads[, id]) in the
    order of their first records (the id, when given, is the first-record id: the dictionary's insertion order); reads / bad = (pos, end,
    length), broken = (pos, end, length, mate position), each sorted as the buffer keeps it; longest = the three tables' longest reads
    (default: what the tables hold); merge_status / n_cands override cand_n[2g + 1] / cand_n[2g]."""
    contig_len = ref_seq_start + len(ref) if contig_len is None else contig_len
    return dict(ref=bytes(ref), cands=[tuple(c) for c in cands], start=start, end=contig_len if end is None else end, rlen=rlen,
                ref_seq_start=ref_seq_start, contig_len=contig_len, reads=list(reads), bad=list(bad), broken=list(broken), longest=longest, name=name,
                merge_status=merge_status, n_cands=n_cands)


@functools.lru_cache(maxsize=None)
def _base_options():
    return default_options()


def _rem_pos(pos, nrem, nadd):
    """Contig coordinate of the removed bases of a record at refPos `pos`: a deletion is labelled with the base before it."""
    return pos + 1 if (nrem and not nadd) else pos


def _longest(reg):
    if reg["longest"] is not None:
        return list(reg["longest"])
    return [max([r[1] - r[0] for r in t], default=0) for t in (reg["reads"], reg["bad"], reg["broken"])]


def pack(regions, cap_per_scan=None):
    """Arguments of Engine.stage_b for hand-made candidates: dict(regions, tables, cand, cand_n, read_seq, cap_per_scan)."""
    cap = cap_per_scan or max([len(g["cands"]) for g in regions] + [1])
    cand = np.full((len(regions), cap, 8), -7, dtype=np.int32)
    cand_n = np.zeros((len(regions), 2), dtype=np.int32)
    blob, roff = bytearray(b"NN"), 0                                         # (offset 0 is never a record's: a wrong offset shows)
    for g, reg in enumerate(regions):
        for i, c in enumerate(reg["cands"][:cap]):
            pos, nrem, added, supp = c[:4]
            rid = c[4] if len(c) > 4 else i
            cand[g, i] = [rid, supp, supp, pos, nrem, len(added), roff + _rem_pos(pos, nrem, len(added)) - reg["ref_seq_start"] if nrem else -1,
                          len(blob) if added else -1]
            blob += added
        cand_n[g] = [len(reg["cands"]) if reg["n_cands"] is None else reg["n_cands"], reg["merge_status"]]
        roff += len(reg["ref"])
    pos, end, length, mate, tb, tn, tl = [], [], [], [], [], [], []
    for reg in regions:
        lg = _longest(reg)
        for k, t in enumerate((reg["reads"], reg["bad"], reg["broken"])):
            tb.append(len(pos)); tn.append(len(t)); tl.append(lg[k])
            for r in t:
                pos.append(r[0]); end.append(r[1]); length.append(r[2]); mate.append(r[3] if k == 2 else -1)
    base = min([b for b, n in zip(tb[2::3], tn[2::3]) if n] + [len(pos)])     # the mate positions start at the first brokenMates read
    tables = dict(read_off=np.concatenate([[0], np.cumsum(length)]).astype(np.int64), read_pos=pos, read_end=end, tab_begin=tb, tab_n=tn, tab_longest=tl,
                  broken_mate_pos=mate[base:], broken_base=base)
    gs = [dict(ref=reg["ref"], ref_seq_start=reg["ref_seq_start"], contig_len=reg["contig_len"], start=reg["start"], end=reg["end"], rlen=reg["rlen"])
          for reg in regions]
    return dict(regions=gs, tables=tables, cand=cand, cand_n=cand_n, read_seq=bytes(blob), cap_per_scan=cap)


class WindowFasta:
    """The contig as the device sees it: its length and the bytes of one window.  getSequence / getCharacter as hostapi.FastaFile."""

    def __init__(self, name, ref, ref_seq_start, contig_len):
        self.name, self.ref, self.rss, self.n = name, bytes(ref), ref_seq_start, contig_len
        self.refs = {name: SimpleNamespace(SeqLength=contig_len)}

    def getSequence(self, seqName, beginPos, endPos):
        beginPos, endPos = max(0, beginPos), min(self.n - 1, endPos)
        if endPos < beginPos:
            raise IndexError("Cannot have beginPos = %s, endPos = %s" % (beginPos, endPos))
        assert self.rss <= beginPos and endPos <= self.rss + len(self.ref), "the mirror reads outside the reference window"
        return self.ref[beginPos - self.rss:endPos - self.rss]

    def getCharacter(self, seqName, pos):
        if pos >= self.n or pos < 0:
            return b"-"
        assert self.rss <= pos < self.rss + len(self.ref)
        return self.ref[pos - self.rss:pos - self.rss + 1]


def _variants(reg, fasta):
    out = []
    for c in reg["cands"]:
        pos, nrem, added, supp = c[:4]
        pos = max(pos, 0)
        at = _rem_pos(pos, nrem, len(added)) - reg["ref_seq_start"]
        v = H.Variant(reg["name"], pos, reg["ref"][at:at + nrem] if nrem else b"", added, supp, H.PLATYPUS_VAR)
        assert v.nRemoved == nrem, "the removed bases of a hand-made candidate lie outside its reference window"
        v.rem_pos = _rem_pos(pos, nrem, len(added))
        out.append(v)
    return out


def normalise_flag(reg, pos, nrem, nadd):
    """k_sb_variants, documented in the header: a pure indel at refPos >= 100 whose normalisation window [wmin, wmax) is not inside the
    reference window handed over, or whose tail ref[cut + nrem + 1:] is empty (it sits at the contig's end), is the caller's."""
    if nrem == nadd or (nrem > 0 and nadd > 0) or pos < 100:
        return False
    window = max(nadd, nrem) + reg["rlen"]
    seq_max = reg["contig_len"] - 1
    wmin, wmax = max(1, pos - window), min(pos + window, seq_max)
    lr, cut = wmax - wmin, pos - wmin
    return wmin < reg["ref_seq_start"] or wmax > reg["ref_seq_start"] + len(reg["ref"]) or lr < 1 or cut + nrem + 1 >= lr


def _mask(window_vars, hap):
    return sum(1 << i for i, v in enumerate(window_vars) if any(v is x for x in hap.variants))


def _window(reg, fasta, opts, o, kept, w, buf):
    """One calling window: pointers, the decision, its haplotypes."""
    ws, we, vs = w["startPos"], w["endPos"], w["variants"]
    first = next(i for i, v in enumerate(kept) if v is vs[0])
    assert all(kept[first + i] is v for i, v in enumerate(vs)), "a window's variants are a run of the region's list"
    out = dict(start=ws, end=we, first=first, n=len(vs), flags=0, ptrs=None, n_haps=0, masks=[], seqs=[])
    flags = 0
    ptrs = []
    for arr, mate in ((buf.reads, False), (buf.badReads, False), (buf.brokenMates, True)):
        try:
            (arr.setWindowPointersBasedOnMatePos if mate else arr.setWindowPointers)(ws, we)
            ptrs += [arr.windowStart, arr.windowEnd]
        except RuntimeError:                                                    # "Read start pointer > read end pointer": the reference raises
            flags = SBW_HOST
            ptrs += [None, None]
    out["ptrs"] = ptrs
    n_good = (ptrs[1] - ptrs[0]) if ptrs[0] is not None else 0
    rss, n_ref, clen, rlen = reg["ref_seq_start"], len(reg["ref"]), reg["contig_len"], reg["rlen"]
    hap_start, hap_end, end_buf = max(ws, 0), min(we, clen - 1), min(2 * rlen, 500)
    lo, hi = max(hap_start - end_buf, 0), min(hap_end + end_buf, clen - 1)
    if lo < rss or hi > rss + n_ref or any(not (rss <= v.refPos < rss + n_ref) for v in vs):
        flags = SBW_HOST                                                        # the reference window must hold every byte a haplotype can take
    out.update(hap_start=hap_start, hap_end=hap_end, end_buf=end_buf, n_good=n_good)
    if flags:
        out["flags"] = flags
        return out
    mk = lambda hv: H.Haplotype(reg["name"], ws, we, hv, fasta, rlen, opts)
    try:
        ref_hap = mk(())
    except Exception:                                                           # too long / beginPos > endPos: logged there, the caller reproduces it
        out["flags"] = SBW_HOST
        return out
    lg = math.log2(o["maxHaplotypes"] - 1)
    if n_good == 0 or n_good > o["maxReads"]:
        flags = SBW_SKIP
    elif len(vs) > o["maxVariants"]:
        flags = SBW_SKIP if o["skipDifficultWindows"] else SBW_HOST
    elif not (len(vs) <= lg or (o["filterVarsByCoverage"] and o["maxVariants"] <= lg)) or len(vs) > SB_MAXCOMB:
        flags = SBW_HOST                                                        # the greedy filter
    if flags:
        out["flags"] = flags
        return out
    try:
        haps = [ref_hap] + [mk(c) for n in range(1, len(vs) + 1) for c in combinations(vs, n) if H.isHaplotypeValid(c)]
    except Exception:
        out["flags"] = SBW_HOST
        return out
    # what the device decides of sorted(haplotypes): the SB_STAGE bytes behind the haplotypes' common prefix
    common = max(0, min(vs[0].refPos, hap_end) - lo)
    dup = False
    for i in range(len(haps)):
        for j in range(i + 1, len(haps)):
            a, b = haps[i].haplotypeSequence[common:], haps[j].haplotypeSequence[common:]
            lm = min(len(a), len(b), SB_STAGE)
            if a[:lm] != b[:lm]:
                continue
            if lm == SB_STAGE and (len(a) > SB_STAGE or len(b) > SB_STAGE):
                dup = True                                                      # they agree on the whole stage and go on
            elif len(a) == len(b):                                              # one sequence: mergeHaplotypes decides by the priors ...
                for h in (haps[i], haps[j]):
                    for v in h.variants:
                        if v.nAdded != v.nRemoved:
                            dup = True                                          # ... which for an indel need the repeat annotation: the caller's
                        elif v.nAdded > 1 and not 1 <= sum(x != y for x, y in zip(v.added, v.removed)) <= 16:
                            dup = True
    if dup:
        out.update(flags=SBW_DUPLICATE, n_haps=len(haps), masks=[_mask(vs, h) for h in haps], seqs=[h.haplotypeSequence for h in haps], ordered=False)
        return out
    merged = H.mergeHaplotypes(haps, fasta)
    if len(merged) <= 1:
        out["flags"] = SBW_SKIP
        return out
    out.update(n_haps=len(merged), masks=[_mask(vs, h) for h in merged], seqs=[h.haplotypeSequence for h in merged], ordered=True)
    return out


def _key_runs(norm):
    """The runs of candidates that compare equal under Variant.__richcmp__'s order, (refPos, type, nRemoved), in a sorted list."""
    runs, i = [], 0
    while i < len(norm):
        e = i + 1
        while e < len(norm) and not (norm[i] < norm[e]):
            e += 1
        runs.append(norm[i:e])
        i = e
    return runs


def _key_run_over(norm, limit):
    """The header's rule of reason 2: "more than 48 candidates with one key count as such" -- the device does not look inside so long a
    run, whatever it holds (caller.order_can_matter, the host's rule, does and lets a run of one variant 49 times pass)."""
    return any(len(r) > limit for r in _key_runs(norm))


def _chain_counts(norm):
    """What the chain did to a region, for the reach conditions of the seeded inputs (not compared with the device): indels whose position
    normalisation changed, runs of equal variants merged, and how many of those hold a moved and an unmoved candidate."""
    moved = lambda v: getattr(v, "given_pos", v.refPos) != v.refPos
    merged = mixed = 0
    for run in _key_runs(norm):
        left = list(run)
        while left:
            same = [v for v in left if v == left[0]]
            left = [v for v in left if not (v == same[0])]
            merged += len(same) >= 2
            mixed += len(same) >= 2 and any(moved(v) for v in same) and not all(moved(v) for v in same)
    return dict(moved=sum(moved(v) for v in norm), merged=merged, mixed=mixed, longest_key_run=max([len(r) for r in _key_runs(norm)], default=0))


def expected_region(reg, o, cp, cap_per_scan, exact_records=None):
    """hdr and content of one region.  exact_records: every distinct record of the scan, in first-record order, as (pos, removed, added,
    index into reg['cands'] or None) -- given when the scan's records are handed to the device (cand_rec): the dictionaries are replayed."""
    out = dict(status=0, reason=0, replay=0, n_records=0, variants=[], windows=[], added_used=0)

    def host(reason):
        out.update(status=PLAT_SB_HOST, reason=reason, variants=[], windows=[], added_used=0)
        return out
    n = len(reg["cands"]) if reg["n_cands"] is None else reg["n_cands"]
    if reg["merge_status"] != 0 or n > SB_CAP or n > cap_per_scan:
        return host(5)                                                          # the merge's own verdict / more candidates than the device holds
    out["n_records"] = sum(c[3] for c in reg["cands"])
    fasta = WindowFasta(reg["name"], reg["ref"], reg["ref_seq_start"], reg["contig_len"])
    opts = copy.copy(_base_options())
    for k in ("minReads", "maxSize", "mergeClusteredVariants", "maxVarDist", "minVarDist", "largeWindows", "maxVariants", "maxHaplotypes"):
        setattr(opts, k, o[k])
    opts.rlen, opts.outputRefCalls = reg["rlen"], 0
    edge = any(normalise_flag(reg, max(c[0], 0), c[1], len(c[2])) for c in reg["cands"])

    def chain(order):
        """sorted -> leftNormaliseIndel -> sorted -> filterVariants over fresh variants in dictionary order `order`."""
        vs = _variants(reg, fasta)
        cands = sorted(vs[i] for i in order)
        norm, fail, used = [], False, 0
        for v in cands:
            try:
                nv = leftNormaliseIndel(v, fasta, reg["rlen"])
            except Exception:                                                   # "Error in variant conversion to standard format"
                fail, nv = True, v
            if nv is not v:
                nv.rem_pos = nv.refPos + 1 if nv.nRemoved else nv.refPos
                nv.moved = True
                nv.given_pos = v.refPos
                used += nv.nAdded                                               # its new bases go into the region's blob right away
            norm.append(nv)
        norm.sort()
        out["normalised"] = [(v.refPos, v.removed, v.added, v.bamMinPos, v.bamMaxPos) for v in norm]  # (before filterVariants adds up the equal ones)
        kept = filterVariants(list(norm), fasta, reg["rlen"], o["minReads"], o["maxSize"], 0, opts)
        return norm, kept, fail, used
    if edge:
        return host(1)
    order = sorted(range(len(reg["cands"])), key=lambda i: reg["cands"][i][4] if len(reg["cands"][i]) > 4 else i)
    norm, kept, fail, used = chain(order)
    # capacities first (reason 6 wins over an exception's 1), then the dictionaries
    if fail or used > cp["cap_added"] or len(kept) > cp["cap_vars"]:
        return host(6 if (used > cp["cap_added"] or len(kept) > cp["cap_vars"]) else 1)
    if caller.order_can_matter(norm, kept) or _key_run_over(norm, SB_KEY_RUN):
        if exact_records is None or len(exact_records) > SB_DICT_CAP:
            return host(2)                                                      # an order that depends on a dictionary, and no records to replay it with (or too many)
        hs = [py2_variant_hash(reg["name"], max(p, 0), r, a) for p, r, a, _ in exact_records]
        first = [k for k in py2_dict_slot_order(hs) if exact_records[k][3] is not None]     # the sample's dictionary walked: who passes enters the second
        second = [first[k] for k in py2_dict_slot_order([hs[x] for x in first])]
        norm, kept, fail, used = chain([exact_records[k][3] for k in second])
        out["replay"] = 1
        if fail or used > cp["cap_added"] or len(kept) > cp["cap_vars"]:
            return host(6 if (used > cp["cap_added"] or len(kept) > cp["cap_vars"]) else 1)
    used += sum(v.nAdded for v in kept if not getattr(v, "moved", False))
    if used > cp["cap_added"]:
        return host(6)
    out["added_used"] = used
    out["chain"] = _chain_counts(norm)
    out["variants"] = [dict(pos=v.refPos, nrem=v.nRemoved, nadd=v.nAdded, added=v.added, removed=v.removed, support=v.nSupportingReads, bam_min=v.bamMinPos,
                            bam_max=v.bamMaxPos, rem_pos=v.rem_pos if v.nRemoved else v.refPos) for v in kept]
    wins = [w for w in WindowGenerator().WindowsAndVariants(reg["name"], reg["start"], reg["end"], reg["contig_len"] - 1, kept, opts)
            if len(w["variants"]) > 0 and w["endPos"] - w["startPos"] <= o["maxSize"]]
    if len(wins) > cp["cap_windows"]:
        return host(6)
    mkr = lambda t, mate: [H.AlignedRead(b"A", b"!", r[0], end=r[1], matePos=r[3] if mate else -1) for r in t]
    buf = H.bamReadBuffer(mkr(reg["reads"], False), mkr(reg["bad"], False), mkr(reg["broken"], True))
    assert [r.pos for r in buf.reads.array] == [r[0] for r in reg["reads"]] and [r.matePos for r in buf.brokenMates.array] == [r[3] for r in reg["broken"]]
    for arr, lg in zip((buf.reads, buf.badReads, buf.brokenMates), _longest(reg)):
        arr.longestRead = lg
    out["windows"] = [_window(reg, fasta, opts, o, kept, w, buf) for w in wins]
    return out


def expected(regions, o, cp, cap_per_scan=None, exact_records=None):
    """Expected content of one plat_stage_b_batch call: per region (expected_region) and the window batch."""
    cap = cap_per_scan or max([len(g["cands"]) for g in regions] + [1])
    regs = [expected_region(g, o, cp, cap, exact_records[k] if exact_records else None) for k, g in enumerate(regions)]
    b = dict(hap_begin=[0], read_begin=[0], pair_off=[0], gl_off=[0], hap_off=[0], read_off=[0], start=[], end=[], flank=[], n_good=[], masks=[], seqs=[],
             read_src=[], read_kind=[], ordered=[])
    base = 0
    read_len = []
    for g in regions:
        read_len += [r[2] for t in (g["reads"], g["bad"], g["broken"]) for r in t]
    tab_begin = []
    for g in regions:
        for t in (g["reads"], g["bad"], g["broken"]):
            tab_begin.append(base)
            base += len(t)
    max_len = max_reads = max_haps = 0
    for k, (g, r) in enumerate(zip(regions, regs)):
        for w in r["windows"]:
            w["batch"] = -1
            if w["flags"] not in (0, SBW_DUPLICATE):
                continue
            w["batch"] = len(b["start"])
            src = [(tab_begin[3 * k + a] + i, a) for a in range(3) for i in range(w["ptrs"][2 * a], w["ptrs"][2 * a + 1])]
            nh, nr = w["n_haps"], len(src)
            b["hap_begin"].append(b["hap_begin"][-1] + nh); b["read_begin"].append(b["read_begin"][-1] + nr)
            b["pair_off"].append(b["pair_off"][-1] + nh * nr); b["gl_off"].append(b["gl_off"][-1] + nh * (nh + 1) // 2)
            b["start"].append(w["hap_start"]); b["end"].append(w["hap_end"]); b["flank"].append(w["end_buf"]); b["n_good"].append(w["n_good"])
            b["masks"].append(w["masks"]); b["seqs"].append(w["seqs"]); b["ordered"].append(w["ordered"])
            for s in w["seqs"]:
                b["hap_off"].append(b["hap_off"][-1] + len(s))
            for i, a in src:
                b["read_src"].append(i); b["read_kind"].append(a); b["read_off"].append(b["read_off"][-1] + read_len[i])
            max_len, max_reads, max_haps = max([max_len] + [len(s) for s in w["seqs"]]), max(max_reads, nr), max(max_haps, nh)
    nw = len(b["start"])
    totals = [nw, b["hap_begin"][-1], b["read_begin"][-1], b["pair_off"][-1], b["gl_off"][-1], b["hap_off"][-1], b["read_off"][-1], max_len, max_reads, max_haps]
    over = nw > cp["cap_batch_windows"] or totals[1] > cp["cap_batch_haps"] or totals[2] > cp["cap_batch_reads"] or totals[5] > cp["cap_hap_bytes"]
    totals.append(1 if over else 0)
    b["totals"] = totals
    return dict(regions=regs, batch=b)


def counts(exp):
    """(regions flagged, windows, windows in the batch, haplotypes in the batch) of an expectation: what a test compared."""
    rs = exp["regions"]
    return dict(regions=len(rs), flagged=sum(r["status"] != 0 for r in rs), variants=sum(len(r["variants"]) for r in rs),
                windows=sum(len(r["windows"]) for r in rs), batch_windows=exp["batch"]["totals"][0], haplotypes=exp["batch"]["totals"][1])


def compare(out, exp, regions, cp, sentinel_of):
    """Assert the arrays Engine.stage_b returned against expected(): every array of every step, by content; and that every element
    behind what the counts say was written still holds the sentinel.  A region flagged PLAT_SB_HOST promises nothing about its own
    slices (the header: "nothing else of the region is valid"); they are only required not to spill (every other region's are checked)."""
    i4, i8, u1, u4 = (sentinel_of(t) for t in ("i4", "i8", "u1", "u4"))
    var_keys = ("var_pos", "var_nrem", "var_nadd", "var_support", "var_bam_min", "var_bam_max", "var_rem_pos", "var_add_off")
    win_keys = ("win_start", "win_end", "win_var_first", "win_var_n", "win_flags", "win_n_haps", "win_batch")
    for g, (reg, e) in enumerate(zip(regions, exp["regions"])):
        hdr = out["hdr"][g].tolist()
        where = "region %d" % g
        assert (hdr[0], hdr[5]) == (e["status"], e["reason"]), (where, "status / reason", hdr, e["status"], e["reason"])
        if e["status"]:
            assert hdr[1] == hdr[2] == 0, (where, hdr)
            continue
        assert hdr[1] == len(e["variants"]), (where, "n_variants", hdr, len(e["variants"]))
        assert hdr[2] == len(e["windows"]), (where, "n_windows", hdr, len(e["windows"]))
        assert hdr[3] == e["n_records"] and hdr[4] == e["added_used"] and hdr[6] == e["replay"] and hdr[7] == 0, (where, "hdr[3,4,6,7]", hdr, e["n_records"], e["added_used"])
        nv, nw = hdr[1], hdr[2]
        spans = []
        for i, v in enumerate(e["variants"]):
            got = {k: int(out[k][g, i]) for k in var_keys}
            at = "%s variant %d" % (where, i)
            for k, x in (("var_pos", "pos"), ("var_nrem", "nrem"), ("var_nadd", "nadd"), ("var_support", "support"), ("var_bam_min", "bam_min"),
                         ("var_bam_max", "bam_max"), ("var_rem_pos", "rem_pos")):
                if k != "var_rem_pos" or v["nrem"]:                             # (where nothing is removed the coordinate says nothing: not specified)
                    assert got[k] == v[x], (at, k, got, v)
            if v["nadd"]:
                a0 = got["var_add_off"]
                assert 0 <= a0 and a0 + v["nadd"] <= e["added_used"], (at, "var_add_off", got, e["added_used"])
                assert out["added"][g, a0:a0 + v["nadd"]].tobytes() == v["added"], (at, "added bytes", out["added"][g, a0:a0 + v["nadd"]].tobytes(), v["added"])
                spans.append((a0, a0 + v["nadd"]))
            if v["nrem"]:
                r0 = got["var_rem_pos"] - reg["ref_seq_start"]
                assert reg["ref"][r0:r0 + v["nrem"]] == v["removed"], (at, "removed bytes")
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (where, "added bases of two variants overlap", spans)
        for k in var_keys:
            assert (out[k][g, nv:] == i4).all(), (where, k, "written behind n_variants")
        assert (out["added"][g, e["added_used"]:] == u1).all(), (where, "added written behind hdr[4]")
        for i, w in enumerate(e["windows"]):
            at = "%s window %d" % (where, i)
            got = {k: int(out[k][g, i]) for k in win_keys}
            want = dict(win_start=w["start"], win_end=w["end"], win_var_first=w["first"], win_var_n=w["n"], win_flags=w["flags"], win_n_haps=w["n_haps"],
                        win_batch=-1 if exp["batch"]["totals"][10] else w["batch"])
            assert got == want, (at, got, want)
            if None not in w["ptrs"]:
                assert out["win_ptrs"][g, i].tolist() == w["ptrs"], (at, "win_ptrs", out["win_ptrs"][g, i].tolist(), w["ptrs"])
        for k in win_keys:
            assert (out[k][g, nw:] == i4).all(), (where, k, "written behind n_windows")
        assert (out["win_ptrs"][g, nw:] == i4).all(), (where, "win_ptrs written behind n_windows")
    b = exp["batch"]
    tot = out["totals"].tolist()
    assert tot[:11] == b["totals"] and tot[11:] == [0] * 5, ("totals", tot, b["totals"])
    nw, nh, nr = b["totals"][:3]
    if b["totals"][10]:                                                         # a batch capacity was too small: nothing of the batch is written
        nw = nh = nr = 0
        for k in ("b_hap_begin", "b_read_begin", "b_seg_begin"):
            assert (out[k] == i4).all(), k
        for k in ("b_pair_off", "b_gl_off", "b_hap_off", "b_read_off"):
            assert (out[k] == i8).all(), k
        assert all((out["win_batch"][g, :len(e["windows"])] == -1).all() for g, e in enumerate(exp["regions"]) if not e["status"])
    else:
        for k, x in (("b_hap_begin", "hap_begin"), ("b_read_begin", "read_begin"), ("b_seg_begin", "read_begin"), ("b_pair_off", "pair_off"), ("b_gl_off", "gl_off")):
            assert out[k][:nw + 1].tolist() == b[x], (k, out[k][:nw + 1].tolist(), b[x])
            assert (out[k][nw + 1:] == (i8 if out[k].dtype == np.int64 else i4)).all(), (k, "written behind the batch's windows")
        for k, x in (("b_start", "start"), ("b_end", "end"), ("b_flank", "flank"), ("b_n_good", "n_good")):
            assert out[k][:nw].tolist() == b[x], (k, out[k][:nw].tolist(), b[x])
        assert out["b_read_off"][:nr + 1].tolist() == b["read_off"] and (out["b_read_off"][nr + 1:] == i8).all(), "b_read_off"
        assert out["b_read_src"][:nr].tolist() == b["read_src"], ("b_read_src", out["b_read_src"][:nr].tolist(), b["read_src"])
        assert out["b_read_kind"][:nr].tolist() == b["read_kind"], "b_read_kind"
        assert (out["b_hap_off"][nh + 1:] == i8).all(), "b_hap_off written behind the batch's haplotypes"
        off = out["b_hap_off"][:nh + 1].tolist()
        for w in range(nw):
            h0, h1 = b["hap_begin"][w], b["hap_begin"][w + 1]
            got = [(int(out["b_hap_mask"][h]), out["b_hap_seq"][off[h]:off[h + 1]].tobytes()) for h in range(h0, h1)]
            want = list(zip(b["masks"][w], b["seqs"][w]))
            if b["ordered"][w]:
                assert got == want, ("batch window %d" % w, "haplotypes (mask, bytes) in order", [m for m, _ in got], [m for m, _ in want])
                assert [s for _, s in got] == sorted(s for _, s in got)
            else:                                                               # PLAT_SBW_DUPLICATE: every haplotype, the order is the caller's
                assert sorted(got) == sorted(want), ("batch window %d" % w, "haplotypes (mask, bytes) as a set")
        assert off == b["hap_off"] or not all(b["ordered"]), ("b_hap_off", off, b["hap_off"])
        assert off[0] == 0 and off[-1] == b["hap_off"][-1] and [off[b["hap_begin"][w]] for w in range(nw + 1)] == [b["hap_off"][b["hap_begin"][w]] for w in range(nw + 1)]
    for k in ("b_start", "b_end", "b_flank", "b_n_good"):
        assert (out[k][nw:] == i4).all(), (k, "written behind the batch's windows")
    assert (out["b_read_src"][nr:] == i4).all() and (out["b_read_kind"][nr:] == u1).all(), "read arrays written behind the batch's reads"
    assert (out["b_hap_mask"][nh:] == u4).all(), "b_hap_mask written behind the batch's haplotypes"
    assert (out["b_hap_seq"][(0 if b["totals"][10] else b["totals"][5]):] == u1).all(), "b_hap_seq written behind the batch's bytes"


# counts computed from the fixtures (tests/test_stage_b_reference_cpu.py and tests/test_gpu_stage_b_kernels.py assert the same ones)
N_NORMALISE, N_NORMALISE_ELIGIBLE, N_NORMALISE_FLAGGED, N_NORMALISE_MOVED = 1000, 787, 3, 196
N_FILTER_KEPT = 340                                                         # variants the 60 filter_variants lists keep (12 lists flagged)
N_WINDOW_CASES, N_WINDOW_CASES_IN_PLACE, N_WINDOWS_IN_PLACE = 50, 42, 369
N_POINTER_QUERIES = 1200
N_VALID, N_VALID_IN_PLACE = 400, 346
N_HAPSEQ, N_HAPSEQ_GOLDEN_BYTES = 96, 74


def in_place(reg, e):
    """The chain left the region's candidates as they were given: nothing flagged, moved, merged or dropped."""
    return e["status"] == 0 and [(v["pos"], v["nrem"], v["added"], v["support"]) for v in e["variants"]] == [(max(p, 0), n, a, s) for p, n, a, s in (c[:4] for c in reg["cands"])]


# ---- the golden corpora as regions ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def synth_ref(n, seed):
    """A reference without runs: no two neighbours equal and no base equal to the one two places before it, so that no indel placed in it
    can move (neither homopolymers nor dinucleotide repeats) unless a test plants a repeat."""
    bits = np.random.default_rng(seed).integers(0, 2, n).tolist()
    out = [65 + 2 * bits[0] if n else 0, 71 if n > 1 else 0][:n]
    a, b = (out + [0, 0])[:2]
    for i in range(2, n):
        allowed = [c for c in (65, 67, 71, 84) if c != a and c != b]
        a, b = b, allowed[bits[i]]
        out.append(b)
    return bytes(out)


def pin_ref(ref, cands):
    """`ref` with the base at every pure indel's position changed, where needed, so that the indel cannot move to the left (a deletion
    moves when the base before it equals its last base, an insertion when that base equals its last added base), and the base at every
    SNP / MNP position changed so that the variant differs from the reference."""
    ref = bytearray(ref)
    for pos, nrem, added, *_ in sorted(cands, key=lambda c: c[0]):
        if nrem == len(added):
            for i, a in enumerate(added):
                if pos + i < len(ref) and ref[pos + i] == a:
                    ref[pos + i] = next(c for c in b"ACGT" if c != a and (pos + i < 1 or c != ref[pos + i - 1]))
        elif (nrem == 0 or not added) and 0 < pos < len(ref) - nrem - 1:
            last = added[-1] if added else ref[pos + nrem]
            first = added[0] if added else ref[pos + 1]
            if ref[pos] == last:
                ref[pos] = next(c for c in b"ACGT" if c != last and c != ref[pos - 1])
            if ref[pos + nrem + 1] == first and added:
                ref[pos + nrem + 1] = next(c for c in b"ACGT" if c != first and c != ref[pos + nrem])
    return bytes(ref)


def _cand(v, supp=None):
    return (v["pos"], len(v["removed"]), v["added"].encode(), v.get("n_supporting", 2) if supp is None else supp)


def normalise_cases(g):
    """regionprep_cases['left_normalise']: one region per golden variant, the case's contig as the reference window.  -> [(region, variant)]"""
    return [(region(c["ref"].encode(), [_cand(v)], rlen=c["rlen"]), v) for c in g["left_normalise"] for v in c["variants"]]


NORMALISE_OPTIONS = dict(minReads=0, maxSize=100000)
NORMALISE_CAPS = dict(cap_vars=2, cap_windows=2, cap_added=64, cap_batch_windows=4, cap_batch_haps=8, cap_batch_reads=8, cap_hap_bytes=64)


def cover(lo, hi, step=40, length=100):
    """Reads (pos, end, length) every `step` bases over [lo, hi)."""
    return [(p, p + length, length) for p in range(max(1, lo), max(hi, lo + 1), step)]


def filter_cases(g):
    """regionprep_cases['filter_variants'] restricted to the candidates that come from the reads alone (what the device sees), on a
    synthesised reference.  -> [(region, options, the case, indices of the variants used)]"""
    out = []
    for k, c in enumerate(g["filter_variants"]):
        idx = [i for i, v in enumerate(c["variants"]) if v["source"] == H.PLATYPUS_VAR]
        hi = max(v["pos"] + len(v["removed"]) for v in c["variants"]) + 1200
        reg = region(synth_ref(hi, 100 + k), [_cand(c["variants"][i]) for i in idx], rlen=150)
        out.append((reg, options(minReads=c["min_reads"], maxSize=c["max_size"]), c, idx))
    return out


def window_cases(g):
    """regionprep_cases['windows']: the case's region and options over a synthesised reference, the other contig's variants dropped (as
    getVariantsByPos drops them).  -> [(region, options, the case, indices of the variants used)]"""
    out = []
    for k, c in enumerate(g["windows"]):
        idx = [i for i, v in enumerate(c["variants"]) if v.get("chrom", "20") == "20"]
        o = c["options"]
        clen = c["max_contig_pos"] + 1
        hi = min(clen, max([c["variants"][i]["pos"] + len(c["variants"][i]["removed"]) for i in idx] + [c["start"]]) + 2500)
        ps = [c["variants"][i]["pos"] for i in idx]
        cands = [_cand(c["variants"][i], 2) for i in idx]
        reg = region(pin_ref(synth_ref(hi, 200 + k), cands), cands, start=c["start"], end=c["end"], rlen=o["rlen"], contig_len=clen,
                     reads=cover(min(ps + [hi]) - 50, max(ps + [0]) + 50))
        out.append((reg, options(mergeClusteredVariants=o["mergeClusteredVariants"], maxVariants=o["maxVariants"], largeWindows=o["largeWindows"],
                                 maxSize=o["maxSize"], maxVarDist=o["maxVarDist"], minVarDist=o["minVarDist"]), c, idx))
    return out


POINTER_OPTIONS = dict(minVarDist=1 << 24, maxVarDist=1 << 24, maxSize=1 << 24)


def pointer_cases(g):
    """regionprep_cases['read_arrays']: one region per query -- by_pos as `reads` and `badReads`, by_mate as `brokenMates`, and one SNP at the
    query's start in a region [start, end] of a contig that ends at `end`, so that the calling window is the query's interval.
    -> [(region, golden window, golden mate_window, (start, end))]"""
    out = []
    for k, c in enumerate(g["read_arrays"]):
        rd = [(p, e, e - p) for p, e, _ in c["by_pos"]]
        rm = [(p, e, e - p, m) for p, e, m in c["by_mate"]]
        ref = synth_ref(max(q[1] for q in c["queries"]) + 1, 300 + k)
        for (s, e), win, mwin in zip(c["queries"], c["window"], c["mate_window"]):
            base = ref[s:s + 1]
            reg = region(ref[:e + 1], [(s, 1, b"A" if base != b"A" else b"C", 2)], start=s, end=e + 1, rlen=100, reads=rd, bad=rd, broken=rm,
                         longest=[c["longest"], c["longest"], max([r[1] - r[0] for r in rm], default=0)])
            out.append((reg, win, mwin, (s, e)))
    return out


VALID_OPTIONS = dict(maxVarDist=1000, minVarDist=9, maxVariants=8, maxHaplotypes=50)


def valid_cases(cases, tries=40):
    """filter_cases['valid']: the set's variants (positions, lengths, added bases) as the candidates of one region over a reference
    chosen, among `tries` synthesised ones, so that the chain leaves them where they are (no indel can move, none merge) -- when there is
    one.  -> [(region, the case)]"""
    out = []
    for k, c in enumerate(cases):
        cands = [(p, len(r), a.encode(), 2) for p, r, a in c["variants"]]
        reg = None
        for t in range(tries):
            reg = region(pin_ref(synth_ref(700, 1000 * t + k), cands), cands, rlen=100, reads=cover(40, 200))
            e = expected_region(reg, options(**VALID_OPTIONS), caps(), len(cands))
            n_valid = sum(H.isHaplotypeValid(tuple(H.Variant("20", p, b"N" * n, a) for p, n, a, _ in x)) for m in range(1, len(cands) + 1) for x in combinations(cands, m))
            if (e["status"] == 0 and [(v["pos"], v["nrem"], v["added"]) for v in e["variants"]] == [(p, n, a) for p, n, a, _ in cands] and
                    len(e["windows"]) == 1 and e["windows"][0]["flags"] == 0 and e["windows"][0]["n_haps"] == 1 + n_valid):
                break
        out.append((reg, c))
    return out


def hapseq_cases(cases):
    """hapseq_cases with five variants or fewer: a region that starts at the case's window start, with minVarDist chosen so that the window
    ends where the case's does (when the window rules can do that).  -> [(region, options, the case)]"""
    out = []
    for c in cases:
        if len(c["variants"]) > SB_MAXCOMB:
            continue
        ref = c["ref"].encode()
        hi = max(max(v["pos"], v["pos"] + len(v["removed"]) - 1) for v in c["variants"])
        mvd = max(c["end"] - hi, 0) if c["end"] < len(ref) - 1 else len(ref)
        reg = region(ref, [_cand(v, 2) for v in c["variants"]], start=c["start"], end=len(ref), rlen=c["rlen"],
                     reads=cover(max(c["start"], 1), c["end"] + 1, 1000, 50))
        out.append((reg, options(minVarDist=mvd, maxVarDist=1 << 20, maxSize=1 << 20, largeWindows=1, maxHaplotypes=50), c))
    return out
