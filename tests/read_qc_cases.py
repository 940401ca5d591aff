"""Seeded inputs for the front of the fetched, BAM and BGZF region loops -- checkAndTrimRead (k_read_qc, k_read_qc_packed) and the split of
every stream into its two read buffers (k_read_split, k_read_gather) -- at the shapes the 30 streams of tests/golden/readqc_cases.json.gz do
not reach: reads of 0..1000 bases, quality bytes 0..255, options off the goldens' values, every flag, insert sizes at the edges of the three
rules that read them, CIGARs of 0..79 pairs, streams of 0..1025 reads in every verdict pattern around the 64-read waves and the 512-read tiles
of the split, and one stream past the 262 144 reads whose verdict masks the split keeps in LDS.

Plain Python and numpy.  tests/test_read_qc_cases_cpu.py checks on the oracle alone that the inputs reach what they are here for, and holds
the oracle against the CPU stand-in device on them; tests/test_gpu_read_qc_fuzz.py compares the device with the oracle.

A CALL is dict(name, opt, streams): the streams of one plat_read_buffers_batch call and its options.  A stream is a list of read dicts
{seq, qual (bytes), pos, end, mapq, flag, chromID, mateChromID, insertSize, matePos, cigar [[op, length], ...]}: what Engine.read_buffers and
Oracle.check_and_trim take.  A TABLE (table_of) is the same call flattened into the arrays the C entry points take.

In every read the lengths of M, I and S sum to at most the read's length: past that the reference writes behind the read and has no answer."""
import functools

import numpy as np

M_, I_, D_, SKIP_, S_, H_, P_, EQ_, X_ = range(9)                     # CIGAR operations as BAM numbers them

LENGTHS = (0, 1, 2, 3, 7, 20, 63, 64, 65, 129, 150, 151, 250, 641, 1000)
LENGTH_P = np.array([2, 3, 3, 3, 6, 12, 10, 10, 10, 8, 10, 6, 5, 1.2, 0.8])
STREAM_SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025)
PAIR_COUNTS = (0, 1, 2, 7, 32, 33, 79)
PAIR_COUNT_P = np.array([4, 30, 30, 24, 4, 4, 4.0])
MIN_MAP_QUALS = (0, 1, 20, 60, 255)
MIN_BASE_QUALS = (0, 5, 10, 20, 63, 64)
MIN_GOOD_QUAL_BASES = (0, 1, 20, 40, 200)
TRIM_READ_FLANKS = (0, 1, 5, 40, 2000)
SWITCHES = (0, 1, 2)                                                   # the rule is `== 1`: 2 is off
PAIR_FLAGS = (99, 147, 83, 163, 97, 145, 81, 161, 65, 129)            # the ten ordinary flags of a pair
SPECIAL_BITS = (4, 8, 256, 512, 1024)
LONG_READS = 262144 + 700                                              # past the 4096 masks x 64 reads the split keeps in LDS
REASONS = ("LOW_QUAL_BASES", "UNMAPPED_READ", "MATE_UNMAPPED", "MATE_DISTANT", "SMALL_INSERT", "DUPLICATE", "LOW_MAP_QUAL", "SECONDARY")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def pick(rng, seq, cum=None):
    """One of seq, uniformly or by the cumulative weights `cum` (rng.choice is slow on short Python sequences)."""
    return seq[int(rng.integers(len(seq)))] if cum is None else seq[min(int(np.searchsorted(cum, rng.random(), side="right")), len(seq) - 1)]


LENGTH_CUM = np.cumsum(LENGTH_P / LENGTH_P.sum())
PAIR_COUNT_CUM = np.cumsum(PAIR_COUNT_P / PAIR_COUNT_P.sum())


def options(**kw):
    o = dict(minGoodQualBases=20, minMapQual=20, minBaseQual=20, minFlank=10, trimOverlapping=1, trimAdapter=1, trimReadFlank=0,
             trimSoftClipped=1, enabled=[1, 1, 1, 1])
    o.update(kw)
    return o


def qc_args(o):
    """An options dict as the arguments of Engine.read_qc / Engine.read_buffers."""
    return (o["minGoodQualBases"], o["minMapQual"], o["minBaseQual"], o["trimOverlapping"], o["trimAdapter"], o["trimReadFlank"],
            o["trimSoftClipped"], tuple(o["enabled"]))


def consumed(cigar):
    """The bases checkAndTrimRead's soft-clip cursor can pass: the lengths of M, I and S."""
    return sum(ln for op, ln in cigar if op in (M_, I_, S_))


# ---- one read ------------------------------------------------------------------------------------------------------------------------
def make_cigar(rng, L, npairs):
    """npairs pairs whose M, I and S lengths sum to at most L: every operation 0..8, soft clips leading, trailing, behind a hard clip and
    twice, and =, X, N, P or D in front of a soft clip (which does not move the reference's cursor)."""
    if npairs == 0:
        return []
    if npairs == 1:
        return [[pick(rng, (M_, M_, M_, S_, EQ_)), L]] if rng.random() < 0.9 else [[int(rng.integers(0, 9)), min(L, 5)]]
    shape = rng.integers(0, 6)
    if shape == 0:
        ops = [S_] + [M_] * (npairs - 1)
    elif shape == 1:
        ops = [M_] * (npairs - 1) + [S_]
    elif shape == 2:
        ops = [H_, S_] + [M_] * (npairs - 2)
    elif shape == 3:
        ops = [S_] + [M_] * (npairs - 2) + [S_]
    elif shape == 4:
        ops = [pick(rng, (EQ_, X_, SKIP_, P_, D_)), S_] + [M_] * (npairs - 2)
    else:
        ops = [M_] * npairs
    # the middle of a long CIGAR: alternate M with every other operation, keep the clips where the shape put them
    for k in range(2, npairs - 1):
        if k % 2 == 1:
            ops[k] = pick(rng, (I_, D_, SKIP_, P_, EQ_, X_, I_, D_, S_ if rng.random() < 0.1 else I_))
    if shape == 4 and npairs >= 7:                                      # and once more, deep inside the read
        ops[4], ops[5] = pick(rng, (EQ_, X_, SKIP_, P_, D_)), S_
    eats = [k for k, op in enumerate(ops) if op in (M_, I_, S_)]
    budget = L if rng.random() < 0.8 else int(rng.integers(0, L + 1))
    lens = rng.integers(1, 6, len(ops)).tolist()
    if eats:
        if budget >= len(eats):                                         # a composition of the budget into len(eats) positive parts
            cuts = np.sort(rng.choice(np.arange(1, budget), len(eats) - 1, replace=False)) if len(eats) > 1 else np.zeros(0, int)
            parts = np.diff(np.concatenate([[0], cuts, [budget]]))
        else:                                                           # a read shorter than its CIGAR has pairs: lengths of 0 and 1
            parts = np.zeros(len(eats), dtype=int); parts[rng.choice(len(eats), budget, replace=False)] = 1
        for k, p in zip(eats, parts):
            lens[k] = int(p)
    return [[op, ln] for op, ln in zip(ops, lens)]


def make_qual(rng, L, mbq, kind=None):
    """L quality bytes.  kind: None (drawn), 'good' (every byte at or above max(mbq, 5) and below 64)."""
    if L == 0:
        return b""
    if kind == "good":
        return rng.integers(max(mbq, 5), 64, L).astype(np.uint8).tobytes() if mbq < 64 else rng.integers(64, 128, L).astype(np.uint8).tobytes()
    q = np.clip(rng.normal(36, 11, L), 0, 63).astype(np.uint8)
    t = rng.random()
    edge = np.array([0, 1, 2, 3, 4, 5, max(mbq - 1, 0), mbq, 63, 64], dtype=np.uint8)
    if t < 0.22:                                                        # the threshold values, the packed format's edge
        at = rng.integers(0, L, max(1, L // 6)); q[at] = rng.choice(edge, len(at))
    elif t < 0.40:                                                      # exceptions of the packed table that count as good
        at = rng.integers(0, L, max(1, L // 8)); q[at] = rng.integers(64, 128, len(at))
    elif t < 0.60:                                                      # ... and those that are negative as signed chars
        at = rng.integers(0, L, max(1, L // 10)); q[at] = rng.integers(128, 256, len(at))
    elif t < 0.64:
        q[:] = rng.integers(0, 5, L)                                    # a whole read below 5
    elif t < 0.68:
        q[:] = rng.integers(128, 256, L)
    u = rng.random()
    if u < 0.25:
        q[-int(rng.integers(1, 25)):] = rng.integers(0, 5)              # a low-quality tail, a low-quality head
    elif u < 0.5:
        q[:int(rng.integers(1, 25))] = rng.integers(1, 5)
    elif u < 0.56:
        q[-1] = pick(rng, (130, 200, 255)); q[0] = pick(rng, (128, 129, 254))      # a "negative" byte at the end the tail rule reads
    return q.tobytes()


def insert_sizes(L):
    e = [0, 1, -1, L - 1, -(L - 1), L, -L, L + 1, -(L + 1), 2 * L - 1, -(2 * L - 1), 2 * L, -2 * L, 2 * L + 1, -(2 * L + 1),
         100000, -100000, 2 ** 31 - 1, -(2 ** 31 - 1)]
    return e


def make_read(rng, L, pos, opt, npairs=None, accepted=False):
    """One read.  accepted=True: built so that every test of the rule passes under `opt` (mapq, qualities, flag, insert size); the caller
    keeps positions distinct."""
    mbq, mmq = opt["minBaseQual"], opt["minMapQual"]
    if npairs is None:
        npairs = pick(rng, PAIR_COUNTS, PAIR_COUNT_CUM)
    seq = ACGT[rng.integers(0, 4, L)].copy()
    if L and rng.random() < 0.15:
        seq[rng.integers(0, L, max(1, L // 20))] = ord("N")
    if accepted:
        qual = make_qual(rng, L, mbq, "good") if rng.random() < 0.5 else None
        if qual is None:                                                # good enough, with tails, clips and exceptions to trim and to keep
            q = np.frombuffer(make_qual(rng, L, mbq, "good"), dtype=np.uint8).copy()
            spare = L - max(opt["minGoodQualBases"], 0)
            if spare > 0:
                k = int(rng.integers(0, min(spare, 12) + 1))
                if k:
                    side = rng.random()
                    vals = rng.choice(np.array([0, 1, 4, 130, 255], dtype=np.uint8), k)
                    if side < 0.5: q[L - k:] = vals
                    else: q[:k] = vals
            qual = q.tobytes()
        mapq = pick(rng, [v for v in (mmq, mmq + 1, 60, 254, 255) if mmq <= v <= 255])
        flag = pick(rng, PAIR_FLAGS[:4] + (0, 16))
        ins = pick(rng, (0, L, -L, L + 1, 2 * L - 1, -(2 * L - 1), 2 * L, 2 * L + 1, 3 * L + 7, -(3 * L + 7), 100000)) if L else 0
        mate_chrom = 1
    else:
        qual = make_qual(rng, L, mbq)
        lo = [v for v in (0, 1, 19, 20, 21, 59, 60, 61, 254, 255, mmq - 1) if 0 <= v < mmq]
        hi = [v for v in (0, 1, 19, 20, 21, 59, 60, 61, 254, 255, mmq, mmq + 1) if mmq <= v <= 255]
        mapq = pick(rng, lo) if lo and rng.random() < 0.07 else pick(rng, hi)
        t = rng.random()
        if t < 0.58:
            flag = pick(rng, PAIR_FLAGS[:4])
        elif t < 0.66:
            flag = pick(rng, PAIR_FLAGS[4:])
        elif t < 0.76:
            flag = pick(rng, (0, 16))
        elif t < 0.93:                                                  # each special bit alone and in combination, on a pair or alone
            flag = pick(rng, PAIR_FLAGS[:4] + (0, 16))
            for _ in range(pick(rng, (1, 1, 1, 2, 3))):
                flag |= pick(rng, SPECIAL_BITS + (8,))
        else:
            flag = int(rng.integers(0, 2048))
        ins = pick(rng, insert_sizes(L)) if rng.random() < 0.75 else pick(rng, (300, 420, -380, 350))
        mate_chrom = 1 if rng.random() < 0.95 else 2
    cigar = make_cigar(rng, L, npairs)
    return dict(seq=seq.tobytes(), qual=qual, pos=pos, end=pos + L, mapq=mapq, flag=flag, chromID=1, mateChromID=mate_chrom,
                insertSize=ins, matePos=pos + pick(rng, (150, 200, 200)), cigar=cigar)


def clone(read, **kw):
    r = dict(read, cigar=[list(c) for c in read["cigar"]])
    r.update(kw)
    return r


# ---- streams in verdict patterns ---------------------------------------------------------------------------------------------------------
def pattern_stream(rng, n, pos0, opt, rejected, how):
    """n reads that are all accepted, but for those at the indices `rejected`: through a mapq below minMapQual (how = 'mapq') or the
    duplicate flag (how = 'dup').  Positions rise strictly from pos0."""
    out, pos = [], pos0
    lengths = [L for L in LENGTHS if L >= max(opt["minGoodQualBases"], 0)]
    cum = np.cumsum([LENGTH_P[LENGTHS.index(L)] for L in lengths]); cum /= cum[-1]
    for i in range(n):
        pos += int(rng.integers(1, 5))
        r = make_read(rng, pick(rng, lengths, cum), pos, opt, accepted=True)
        if i in rejected:
            if how == "mapq":
                r["mapq"] = int(rng.integers(0, opt["minMapQual"]))
            else:
                r["flag"] |= 1024
        out.append(r)
    return out


PATTERNS = ("all_accepted", "all_rejected", "alternating", "one@0", "one@63", "one@64", "one@511", "one@512", "one@last")


def rejected_of(pattern, n):
    if pattern == "all_accepted":
        return set()
    if pattern == "all_rejected":
        return set(range(n))
    if pattern == "alternating":
        return set(range(1, n, 2))
    k = pattern.split("@")[1]
    k = n - 1 if k == "last" else int(k)
    return {k} if 0 <= k < n else None


def pattern_calls():
    """Every stream size in every verdict pattern that exists at it, in three calls of mixed sizes with empty streams first, last and side by
    side; where one stream ends accepted and the next begins accepted, the next one's first read is an exact copy of that last read: a
    duplicate by position, length and mate position that the rule must NOT see, because theLastRead starts at NULL in every stream."""
    rng = np.random.default_rng(97531)
    opts = [options(minGoodQualBases=0, minMapQual=20, minBaseQual=10, trimReadFlank=0, trimOverlapping=1, trimAdapter=2, trimSoftClipped=1),
            options(minGoodQualBases=1, minMapQual=60, minBaseQual=5, trimReadFlank=1, trimOverlapping=2, trimAdapter=1, trimSoftClipped=0),
            options(minGoodQualBases=1, minMapQual=1, minBaseQual=20, trimReadFlank=5, trimOverlapping=0, trimAdapter=1, trimSoftClipped=1)]
    todo = [(n, p) for n in STREAM_SIZES for p in PATTERNS if rejected_of(p, n) is not None and (n in (65, 513, 1025) if "@" in p else n > 0 or p == "all_accepted")]
    todo = [todo[k] for k in rng.permutation(len(todo))]
    calls = []
    for c, opt in enumerate(opts):
        streams, labels, pos = [[]], ["empty"], 1000
        mine = todo[c::3]
        for k, (n, pattern) in enumerate(mine):
            how = "mapq" if (k + c) % 2 == 0 else "dup"
            st = pattern_stream(rng, n, pos, opt, rejected_of(pattern, n), how)
            prev = streams[-1]
            if st and prev and 0 not in rejected_of(pattern, n) and prev[-1]["mapq"] >= opt["minMapQual"] and not prev[-1]["flag"] & 1024:
                st[0] = clone(prev[-1])
                labels.append("%d:%s:%s:copies_last" % (n, pattern, how))
            else:
                labels.append("%d:%s:%s" % (n, pattern, how))
            streams.append(st)
            if st:
                pos = st[-1]["pos"]
            if k % 7 == 3:
                streams += [[], []]; labels += ["empty", "empty"]
        streams.append([]); labels.append("empty")
        calls.append(dict(name="patterns%d" % c, opt=opt, streams=streams, labels=labels))
    # one unsorted stream, and one whose only descent lies between the last read of one 512-read tile and the first of the next
    opt = opts[0]
    uns = pattern_stream(rng, 200, 5000, opt, set(), "mapq")
    for r in uns[50:60]:
        r["pos"] -= 40; r["end"] -= 40
    seam = pattern_stream(rng, 700, 9000, opt, set(range(0, 700, 5)), "dup")
    shift = seam[511]["pos"] - seam[0]["pos"] + 3
    for r in seam[512:]:
        r["pos"] -= shift; r["end"] -= shift
    assert [i for i in range(1, 700) if seam[i]["pos"] < seam[i - 1]["pos"]] == [512]
    calls.append(dict(name="order", opt=opt, streams=[uns, seam, pattern_stream(rng, 64, 20000, opt, set(), "mapq")],
                      labels=["unsorted", "descent@512", "64:sorted"]))
    return calls


# ---- streams drawn at random ---------------------------------------------------------------------------------------------------------------
def fuzz_options(rng):
    w = lambda vals, p: vals[int(rng.choice(len(vals), p=np.array(p, dtype=float) / sum(p)))]
    return options(minMapQual=w(MIN_MAP_QUALS, [3, 3, 5, 3, 1]), minBaseQual=w(MIN_BASE_QUALS, [3, 4, 5, 5, 1, 1]),
                   minGoodQualBases=w(MIN_GOOD_QUAL_BASES, [6, 6, 5, 2, 1]), trimReadFlank=w(TRIM_READ_FLANKS, [8, 3, 4, 2, 1]),
                   trimOverlapping=w(SWITCHES, [3, 4, 1]), trimAdapter=w(SWITCHES, [3, 4, 1]), trimSoftClipped=w(SWITCHES, [3, 4, 1]),
                   enabled=None)


def fuzz_stream(rng, n, pos, opt):
    out = []
    for i in range(n):
        if rng.random() > 0.12:
            pos += int(rng.integers(0, 4))
        t = rng.random()
        if out and t < 0.10:                                            # the previous read's position and length again
            prev = out[-1]
            r = make_read(rng, len(prev["seq"]), prev["pos"], opt)
            r["flag"] = prev["flag"] & 1 | (r["flag"] & ~1 & ~0x704 & ~8) | (2 if prev["flag"] & 1 else 0)
            r["mateChromID"] = 1
            r["matePos"] = prev["matePos"] if rng.random() < 0.6 else prev["matePos"] + 7
            r["insertSize"] = pick(rng, (0, 4000))
        elif out and t < 0.13:                                          # the same position with another length
            prev = out[-1]
            r = make_read(rng, pick(rng, [L for L in LENGTHS if L != len(prev["seq"])]), prev["pos"], opt)
            r["matePos"] = prev["matePos"]
        else:
            L = pick(rng, LENGTHS, LENGTH_CUM)
            r = make_read(rng, L, pos, opt, accepted=rng.random() < 0.45)
        out.append(r)
    return out


def fuzz_calls():
    """Calls of 1..4 streams with options drawn from the lists above, all 16 settings of `enabled` in turn."""
    rng = np.random.default_rng(86420)
    calls = []
    for c in range(48):
        opt = fuzz_options(rng)
        opt["enabled"] = [(c >> k) & 1 for k in range(4)] if c < 16 else [int(rng.random() < 0.8) for _ in range(4)]
        if c % 8 == 5:                                                  # the values drawn seldom, each in a call of its own
            key, val = (("minBaseQual", 63), ("minBaseQual", 64), ("minMapQual", 255), ("minGoodQualBases", 200), ("trimReadFlank", 2000),
                        ("trimReadFlank", 40))[c // 8]
            opt[key] = val
        streams, pos = [], 1000
        for s in range(int(rng.integers(1, 5))):
            st = fuzz_stream(rng, int(rng.integers(20, 130)), pos, opt)
            streams.append(st)
            pos = st[-1]["pos"] + 1
        calls.append(dict(name="fuzz%d" % c, opt=opt, streams=streams, labels=["fuzz"] * len(streams)))
    return calls


@functools.lru_cache(maxsize=None)
def calls():
    """Every call but the long stream.  Cached: treat the result as read-only (the oracle and table_of copy what they are given)."""
    return pattern_calls() + fuzz_calls()


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
def table_of(streams):
    """The streams of one call flattened: the arrays of plat_readqc_batch / plat_read_buffers_in (offsets from 0, with their closing entry)."""
    reads = [r for st in streams for r in st]
    arr = lambda k, dt: np.array([r[k] for r in reads], dtype=dt)
    blob = lambda k: np.frombuffer(b"".join(r[k] for r in reads), dtype=np.uint8).copy()
    return dict(seq=blob("seq"), qual=blob("qual"),
                off=np.concatenate([[0], np.cumsum([len(r["qual"]) for r in reads])]).astype(np.int64),
                pos=arr("pos", np.int32), end=arr("end", np.int32), mapq=arr("mapq", np.uint8), flags=arr("flag", np.int32),
                cid=arr("chromID", np.int16), mcid=arr("mateChromID", np.int16), ins=arr("insertSize", np.int32), mpos=arr("matePos", np.int32),
                cig=np.array([x for r in reads for c in r["cigar"] for x in c], dtype=np.int16).reshape(-1),
                coff=np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])]).astype(np.int32),
                sbeg=np.concatenate([[0], np.cumsum([len(st) for st in streams])]).astype(np.int32))


def concat_tables(tabs):
    """Tables one behind the other as the streams of one call."""
    out = {k: np.concatenate([t[k] for t in tabs]) for k in ("seq", "qual", "pos", "end", "mapq", "flags", "cid", "mcid", "ins", "mpos", "cig")}
    for k, dt in (("off", np.int64), ("coff", np.int32), ("sbeg", np.int32)):
        parts, base = [np.zeros(1, dtype=dt)], 0
        for t in tabs:
            parts.append((t[k][1:] + base).astype(dt)); base += int(t[k][-1])
        out[k] = np.concatenate(parts)
    return out


def stream_slice(tab, s):
    """Stream s of a table as the arguments of Oracle.check_and_trim_arrays (offsets from 0)."""
    a, z = int(tab["sbeg"][s]), int(tab["sbeg"][s + 1])
    b0, b1, c0, c1 = int(tab["off"][a]), int(tab["off"][z]), int(tab["coff"][a]), int(tab["coff"][z])
    return (tab["qual"][b0:b1], tab["off"][a:z + 1] - b0, tab["pos"][a:z], tab["mapq"][a:z], tab["flags"][a:z], tab["cid"][a:z], tab["mcid"][a:z],
            tab["ins"][a:z], tab["mpos"][a:z], tab["cig"][2 * c0:2 * c1], tab["coff"][a:z + 1] - c0)


def oracle_table(oracle, tab, opt):
    """checkAndTrimRead over a table, stream by stream as bamReadBuffer sees them: (ok, reason, flags_out, qual_out) of the whole table."""
    n = len(tab["pos"])
    ok, why, flags, qual = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(len(tab["qual"]), np.uint8)
    for s in range(len(tab["sbeg"]) - 1):
        a, z = int(tab["sbeg"][s]), int(tab["sbeg"][s + 1])
        if z > a:
            ok[a:z], flags[a:z], qual[int(tab["off"][a]):int(tab["off"][z])], why[a:z] = oracle.check_and_trim_arrays(*stream_slice(tab, s), opt)
    return ok, why, flags, qual


@functools.lru_cache(maxsize=None)
def long_table():
    """One stream of LONG_READS reads of 1..3 bases, built as arrays: positions never fall, about 40 % rejected in an irregular pattern
    (duplicate flag or a mapq below 20).  Its options: long_options()."""
    rng = np.random.default_rng(13579)
    n = LONG_READS
    lens = rng.integers(1, 4, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nb = int(off[-1])
    # runs of irregular length, so that no tile of 512 reads or wave of 64 looks like its neighbour
    u = rng.random(n)
    burst = np.repeat(rng.random(n // 37 + 1) < 0.3, 37)[:n]
    rej = (u < 0.25) | (burst & (u < 0.75))
    by_mapq = rej & (rng.random(n) < 0.5)
    flags = np.where(rng.random(n) < 0.5, 0, 16).astype(np.int32) | np.where(rej & ~by_mapq, 1024, 0).astype(np.int32)
    mapq = np.where(by_mapq, rng.integers(0, 20, n), rng.integers(20, 256, n)).astype(np.uint8)
    pos = (1000 + 2 * np.arange(n) + np.cumsum(rng.integers(0, 2, n))).astype(np.int32)         # strictly rising: no duplicates by position
    ncig = rng.integers(0, 3, n)
    coff = np.concatenate([[0], np.cumsum(ncig)]).astype(np.int32)
    cig = np.zeros((int(coff[-1]), 2), dtype=np.int16)
    first = coff[:-1][ncig > 0]
    cig[first, 0], cig[first, 1] = M_, lens[ncig > 0]                   # M of the whole read, then (sometimes) a deletion
    second = coff[:-1][ncig > 1] + 1
    cig[second, 0], cig[second, 1] = D_, rng.integers(1, 9, len(second))
    qual = rng.integers(5, 64, nb).astype(np.uint8)
    qual[rng.random(nb) < 0.1] = rng.integers(0, 5)                     # something to trim at the ends
    return dict(seq=ACGT[rng.integers(0, 4, nb)].copy(), qual=qual, off=off, pos=pos, end=(pos + lens).astype(np.int32), mapq=mapq, flags=flags,
                cid=np.ones(n, np.int16), mcid=np.ones(n, np.int16), ins=np.zeros(n, np.int32), mpos=(pos + 200).astype(np.int32),
                cig=cig.reshape(-1), coff=coff, sbeg=np.array([0, n], dtype=np.int32))


def long_options():
    return options(minGoodQualBases=1, minMapQual=20, minBaseQual=5, trimReadFlank=0, trimOverlapping=1, trimAdapter=1, trimSoftClipped=1)


# ---- what a read buffer must hold, from verdicts ----------------------------------------------------------------------------------------------
def expected_split(tab, ok, reason):
    """bamReadBuffer.addReadToBuffer's two buffers of every stream from given verdicts, as plat_read_buffers_batch lays them out: perm (accepted
    reads in order, then rejected ones), counts [10 per stream], the offset tables t_off / t_cigoff [n + 2 per stream], and the order-of-perm
    gather indices of the bytes and the CIGAR shorts."""
    n, ns = len(tab["pos"]), len(tab["sbeg"]) - 1
    lens, pairs = np.diff(tab["off"]), np.diff(tab["coff"]).astype(np.int64)
    perm, counts = np.zeros(n, np.int32), np.zeros(10 * ns, np.int32)
    t_off, t_cig = np.zeros(n + 2 * ns, np.int64), np.zeros(n + 2 * ns, np.int32)
    for s in range(ns):
        a, z = int(tab["sbeg"][s]), int(tab["sbeg"][s + 1])
        idx = np.arange(a, z)
        g, b = idx[ok[a:z] != 0], idx[ok[a:z] == 0]
        perm[a:z] = np.concatenate([g, b])
        counts[10 * s], counts[10 * s + 1] = len(g), int((np.diff(tab["pos"][a:z].astype(np.int64)) < 0).any())
        counts[10 * s + 2:10 * s + 10] = np.bincount(reason[b], minlength=8)
        o = a + 2 * s
        t_off[o:o + len(g) + 1] = np.concatenate([[0], np.cumsum(lens[g])])
        t_off[o + len(g) + 1:o + (z - a) + 2] = np.concatenate([[0], np.cumsum(lens[b])])
        t_cig[o:o + len(g) + 1] = np.concatenate([[0], np.cumsum(pairs[g])])
        t_cig[o + len(g) + 1:o + (z - a) + 2] = np.concatenate([[0], np.cumsum(pairs[b])])

    def gather(starts, counts_):
        dst = np.concatenate([[0], np.cumsum(counts_)])
        return np.repeat(starts - dst[:-1], counts_) + np.arange(int(dst[-1]))
    return dict(perm=perm, counts=counts, t_off=t_off, t_cigoff=t_cig, byte_index=gather(tab["off"][:-1][perm], lens[perm]),
                short_index=gather(2 * tab["coff"][:-1].astype(np.int64)[perm], 2 * pairs[perm]))
