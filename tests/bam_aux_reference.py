"""TEST INFRASTRUCTURE: the read-group rule of plat_bam_route_batch restated in plain Python, from the SAM/BAM specification (section
4.2.4) and the reference loader's use of it (bam_aux_get(b, "RG"), bam_aux2Z, samplesByID[rgID]) -- never from the code under test.
Slices and dict look-ups, no hashing, no cursor arithmetic shared with csrc/bam_aux.hpp.  Also the hand-made records both test files
run and the expected routing of a batch (numpy's stable argsort)."""
import struct

import numpy as np

ROUTED, NO_RG, RG_NOT_STRING, NOT_IN_TABLE, UNKNOWN_TYPE, NEGATIVE_COUNT, AUX_OVERRUN, FIXED_OVERRUN = range(8)
REASONS = ("routed", "no RG field", "RG is no string", "not in the table", "unknown type", "negative count", "aux runs past the record",
           "fixed part runs past the record")

FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
SUBTYPES = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def verdict(rec, table):
    """rec: the record's bytes from refID to its end (block_size bytes); table: {ID bytes: sample}, the integrator's dict.  Returns
    (ROUTED, sample) or (refusal, -1)."""
    rec = bytes(rec)
    if len(rec) < 32:
        return FIXED_OVERRUN, -1
    l_name, n_cig, l_seq = rec[8], struct.unpack_from("<H", rec, 12)[0], struct.unpack_from("<I", rec, 16)[0]
    start = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    if start > len(rec):
        return FIXED_OVERRUN, -1
    aux = rec[start:]
    while len(aux) >= 3:
        tag, typ, rest = aux[:2], chr(aux[2]), aux[3:]
        if tag == b"RG":
            if typ not in "ZH":
                return RG_NOT_STRING, -1
            if b"\0" not in rest:
                return AUX_OVERRUN, -1
            value = rest[:rest.index(b"\0")]
            return (ROUTED, table[value]) if value in table else (NOT_IN_TABLE, -1)
        if typ in "ZH":
            if b"\0" not in rest:
                return AUX_OVERRUN, -1
            aux = rest[rest.index(b"\0") + 1:]
        elif typ == "B":
            if len(rest) < 5:
                return AUX_OVERRUN, -1
            sub, count = chr(rest[0]), struct.unpack_from("<i", rest, 1)[0]
            if sub not in SUBTYPES:
                return UNKNOWN_TYPE, -1
            if count < 0:
                return NEGATIVE_COUNT, -1
            if count * SUBTYPES[sub] > len(rest) - 5:
                return AUX_OVERRUN, -1
            aux = rest[5 + count * SUBTYPES[sub]:]
        elif typ in FIXED:
            if FIXED[typ] > len(rest):
                return AUX_OVERRUN, -1
            aux = rest[FIXED[typ]:]
        else:
            return UNKNOWN_TYPE, -1
    return NO_RG, -1


def table_of(ids, samples):
    """The integrator's dict of a group list; of equal IDs the first one counts (the device: the lowest index wins)."""
    t = {}
    for i, s in zip(ids, samples):
        t.setdefault(bytes(i), int(s))
    return t


def expected_route(verdicts, stream_begin, n_samples):
    """What plat_bam_route_batch leaves for records with these (verdict, sample) pairs: (perm -- the input indices in output order --,
    out_begin [n_streams * n_samples + 1], rec_sample, status [4])."""
    v = np.array([a for a, _ in verdicts], dtype=np.int64).reshape(-1)
    smp = np.array([b for _, b in verdicts], dtype=np.int64).reshape(-1)
    n_streams = len(stream_begin) - 1
    stream_of = np.repeat(np.arange(n_streams), np.diff(stream_begin)).astype(np.int64)
    key = stream_of * n_samples + smp
    ok = np.nonzero(v == ROUTED)[0]
    perm = ok[np.argsort(key[ok], kind="stable")]
    counts = np.bincount(key[ok], minlength=n_streams * n_samples) if len(ok) else np.zeros(n_streams * n_samples, dtype=np.int64)
    out_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    bad = np.nonzero(v != ROUTED)[0]
    status = [-9 if len(bad) else 0, int(bad[0]) if len(bad) else -1, len(ok), len(bad)]
    return perm, out_begin, np.where(v == ROUTED, smp, -1).astype(np.int32), status


# ---- records by hand ------------------------------------------------------------------------------------------------------------
def fixed_part(l_seq=5, n_cig=1, name=b"q\0", pos=100):
    """A record's bytes in front of its aux area (refID 0, one M operation per CIGAR word, bases A, quality 30)."""
    core = struct.pack("<iiBBHHHiiii", 0, pos, len(name), 60, 0, n_cig, 3, l_seq, 0, pos + 50, 150)
    return core + name + struct.pack("<I", (l_seq << 4) | 0) * n_cig + bytes([0x11]) * ((l_seq + 1) // 2) + bytes([30]) * l_seq


def field(tag, typ, value=b""):
    return tag + typ + value


# one field of every type of the specification, and one B array of every subtype
TWELVE = [field(b"XA", b"A", b"x"), field(b"Xc", b"c", b"\xff"), field(b"XC", b"C", b"\x07"), field(b"Xs", b"s", b"\x01\x80"),
          field(b"XS", b"S", b"\x01\x02"), field(b"Xi", b"i", b"\xff\xff\xff\xff"), field(b"XI", b"I", b"RG\0Z"),
          field(b"Xf", b"f", struct.pack("<f", 1.5)), field(b"Xd", b"d", struct.pack("<d", -2.5)), field(b"XZ", b"Z", b"RGZa text\0"),
          field(b"XH", b"H", b"1AE301\0"), field(b"XB", b"B", b"S" + struct.pack("<iHH", 2, 7, 8))]
ARRAYS = [field(b"Y" + s.encode(), b"B", s.encode() + struct.pack("<i", 3) + bytes(range(1, 1 + 3 * n))) for s, n in SUBTYPES.items()]
ARRAYS.append(field(b"Y0", b"B", b"c" + struct.pack("<i", 0)))                     # an empty array

IDS = [b"grpA", b"grpAB", b"g", b"lane.7-x", b"grpA"]                                # a prefix pair, a one-byte ID, a duplicate
SAMPLES = [0, 1, 2, 1, 2]                                                          # (the duplicate's first entry counts: sample 0)


def rg(value, typ=b"Z"):
    return field(b"RG", typ, value + b"\0")


def hand_records():
    """[(name, record bytes)]: the cases of the issue, each a whole record."""
    f = fixed_part()
    out = [("RG first", f + rg(b"grpA") + b"".join(TWELVE)),
           ("RG last", f + b"".join(TWELVE) + b"".join(ARRAYS) + rg(b"grpAB")),
           ("RG alone, type H", f + rg(b"lane.7-x", b"H")),
           ("duplicate RG: the first decides", f + rg(b"g") + rg(b"grpAB")),
           ("duplicate RG: the first is unknown", f + rg(b"nobody") + rg(b"grpA")),
           ("RG of type i", f + field(b"RG", b"i", b"\1\0\0\0") + rg(b"grpA")),
           ("RG of type A behind a field", f + TWELVE[0] + field(b"RG", b"A", b"g")),
           ("an empty value", f + rg(b"")),
           ("a prefix of an ID", f + rg(b"grp")),
           ("an ID that is a prefix of another", f + rg(b"grpA")),
           ("the longer of the two", f + rg(b"grpAB")),
           ("an ID with a byte more", f + rg(b"grpABC")),
           ("no aux data", f),
           ("no RG field", f + b"".join(TWELVE)),
           ("two stray bytes behind the last field", f + TWELVE[0] + b"RG"),
           ("unknown type", f + field(b"XQ", b"Q", b"\0\0") + rg(b"grpA")),
           ("unknown B subtype", f + field(b"XB", b"B", b"d" + struct.pack("<i", 1) + bytes(8)) + rg(b"grpA")),
           ("negative B count", f + field(b"XB", b"B", b"c" + struct.pack("<i", -1)) + rg(b"grpA")),
           ("B count past the end", f + field(b"XB", b"B", b"I" + struct.pack("<i", 0x7fffffff)) + rg(b"grpA")),
           ("B header cut", f + field(b"XB", b"B", b"c\1\0")),
           ("Z without NUL", f + field(b"XZ", b"Z", b"no end")),
           ("RG without NUL", f + b"RGZgrpA"),
           ("i cut", f + field(b"Xi", b"i", b"\1\2\3")),
           ("an odd number of bases and no CIGAR", fixed_part(l_seq=7, n_cig=0, name=b"\0") + rg(b"g")),
           ("a long name and three CIGAR words", fixed_part(l_seq=33, n_cig=3, name=b"n" * 254 + b"\0") + TWELVE[9] + rg(b"lane.7-x")),
           ("the fixed part ends with the record", fixed_part()),
           ("the qualities are cut", fixed_part()[:-1]),
           ("31 bytes", fixed_part()[:31]),
           ("l_seq negative", fixed_part()[:16] + struct.pack("<i", -1) + fixed_part()[20:] + rg(b"grpA"))]
    for i, x in enumerate(TWELVE):
        out.append(("RG behind type %s" % chr(x[2]), f + x + rg(IDS[i % 4])))
    for x in ARRAYS:
        out.append(("RG behind B:%s" % chr(x[3]), f + x + rg(b"grpAB")))
    return out


def record_200():
    """A 200-byte record whose RG field comes last, for the truncations and the mutations."""
    f = fixed_part(l_seq=40, n_cig=2, name=b"read/1\0")
    body = f + TWELVE[9] + TWELVE[11] + TWELVE[5] + ARRAYS[4] + TWELVE[10] + field(b"XA", b"A", b"!")
    tail = rg(b"lane.7-x")
    pad = 200 - len(body) - len(tail)
    assert pad >= 4
    rec = body + field(b"PZ", b"Z", b"p" * (pad - 4) + b"\0") + tail
    assert len(rec) == 200
    return rec, len(f)
