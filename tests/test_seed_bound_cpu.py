"""The seeding proof of k_pairs (platypus_amd/csrc/plat_align.hip, "The seeding stage"), restated in plain Python and held against an exhaustive
diagonal vote (calign.pyx:206-233).  No GPU.

The rule: a lane keeps a set S of tried diagonals -- the union of their U_d (read k-mers that match on d and whose haplotype k-mer occurs once
in the haplotype), the largest count |M_d| of S, its diagonal, and the second largest.  The largest is proven the vote's one arg-max when it
beats the second and `best + |union of U| > nk`, because a diagonal outside S gets at most nk - |union| votes.  S starts with idx0 (hypothesis A),
grows by idx0 +- 1 .. NBR, nearest first, and at the end by hypothesis B's diagonal when that lies further out.  The former rule (PLAT_SEED_ONE_DIAG=1)
proves A or B alone by X < C with X = NUc (maxmult - 1) + (nk - C) maxmult.  A lane still open after B counts, with the no-vote test's look-ups, the
read k-mers that occur nowhere in the haplotype: they vote for nothing and come off the bound."""
import os
import subprocess

import numpy as np

NBR = 20                      # SEED_NBR of plat_align.hip
K = 7


class Hap:
    def __init__(self, seq):
        self.a = np.frombuffer(seq, np.uint8)
        self.n = len(seq)
        self.pos = {}
        for p in range(self.n - K):                                  # the indexed positions, calign.pyx:109
            self.pos.setdefault(seq[p:p + K], []).append(p)
        self.uniq = np.zeros(max(self.n - K, 0), bool)
        for ps in self.pos.values():
            if len(ps) == 1:
                self.uniq[ps[0]] = True
        self.maxmult = max([len(ps) for ps in self.pos.values()] + [1])


def vote(hap, read):
    """The exhaustive vote: {diagonal: count}."""
    cnt = {}
    for i in range(len(read) - K):
        for p in hap.pos.get(read[i:i + K], ()):
            cnt[p - i] = cnt.get(p - i, 0) + 1
    return cnt


def unique_argmax(cnt):
    if not cnt:
        return None
    m = max(cnt.values())
    top = [d for d, c in cnt.items() if c == m]
    return top[0] if len(top) == 1 else None


def marks(hap, ra, d):
    """M_d and U_d as boolean arrays over the read's k-mer starts (d >= 0)."""
    nk = len(ra) - K
    nvalid = min(nk, hap.n - K - d)
    M = np.zeros(nk, bool)
    if nvalid > 0:
        eq = hap.a[d:d + nvalid + K - 1] == ra[:nvalid + K - 1]
        m = eq[:nvalid].copy()
        for j in range(1, K):
            m &= eq[j:nvalid + j]
        M[:nvalid] = m
    U = M.copy()
    if nvalid > 0:
        U[:nvalid] &= hap.uniq[d:d + nvalid]
    return M, U


def old_bound(hap, M, U):
    C, nuc, nk = int(M.sum()), int(M.sum() - U.sum()), len(M)
    return nuc * (hap.maxmult - 1) + (nk - C) * hap.maxmult < C


def hypothesis_b(hap, read):
    for i in range(len(read) - K):
        ps = hap.pos.get(read[i:i + K])
        if ps is not None and len(ps) == 1:
            return ps[0] - i
    return None


def old_rule(hap, read, idx0):
    """A then B, each alone, by X < C.  Returns the proven diagonal or None."""
    ra = np.frombuffer(read, np.uint8)
    if idx0 >= 0 and old_bound(hap, *marks(hap, ra, idx0)):
        return idx0
    d = hypothesis_b(hap, read)
    if d is not None and d != idx0 and d >= 0 and old_bound(hap, *marks(hap, ra, d)):
        return d
    return None


def new_rule(hap, read, idx0, nbr=NBR):
    """The Lemma over the tried set.  Returns (proven diagonal or None, diagonals tried)."""
    ra = np.frombuffer(read, np.uint8)
    nk = len(read) - K
    st = dict(best=-1, bestd=-1, second=-1, orU=np.zeros(nk, bool), tried=0)

    def join(d):
        M, U = marks(hap, ra, d)
        C = int(M.sum())
        st["orU"] |= U
        st["tried"] += 1
        if C > st["best"]:
            st["second"], st["best"], st["bestd"] = st["best"], C, d
        else:
            st["second"] = max(st["second"], C)
        return st["best"] > st["second"] and st["best"] + int(st["orU"].sum()) > nk

    if idx0 >= 0 and join(idx0):
        return st["bestd"], st["tried"]
    for t in range(2 * nbr):
        delta = t // 2 + 1
        d = idx0 - delta if t & 1 else idx0 + delta
        if d >= 0 and join(d):
            return st["bestd"], st["tried"]
    d = hypothesis_b(hap, read)
    if d is not None and d != idx0 and d >= 0 and abs(d - idx0) > nbr and join(d):
        return st["bestd"], st["tried"]
    # the no-vote test's look-ups, counted: a read k-mer that occurs nowhere in the haplotype votes for no diagonal at all
    absent = sum(1 for i in range(nk) if read[i:i + K] not in hap.pos)
    if absent < nk and st["best"] > st["second"] and st["best"] + int(st["orU"].sum()) + absent > nk:
        return st["bestd"], st["tried"]
    return None, st["tried"]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
B = b"ACGT"
READ_LENS = (36, 50, 76, 100, 150, 200, 256)


def rnd(rng, n):
    return bytes(rng.choice(list(B), n).astype(np.uint8))


def substitute(rng, seq, rate=1e-3):
    s = bytearray(seq)
    for p in np.flatnonzero(rng.random(len(s)) < rate):
        s[p] = B[(B.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def indel_pair(rng, hap_len, at, n, repeat_unit=0):
    """(ref, alt): alt carries an insertion (n > 0) or a deletion (n < 0) of |n| bases at `at`.  repeat_unit u > 0: the site lies in a tandem
    repeat of unit u (u = 1: a homopolymer) and the indel is a piece of that repeat, so many diagonals count alike."""
    ref = bytearray(rnd(rng, hap_len))
    if repeat_unit:
        u = rnd(rng, repeat_unit)
        k = int(rng.integers(12, 40))
        ref[at - k // 2:at - k // 2 + k] = (u * k)[:k]
        ins = bytes(ref[at:at + abs(n)]) if abs(n) <= k // 2 else (u * abs(n))[:abs(n)]
    else:
        ins = rnd(rng, abs(n))
    ref = bytes(ref[:hap_len])
    alt = ref[:at] + ins + ref[at:] if n > 0 else ref[:at] + ref[at - n:]
    return ref, alt


def spanning_cases(rng, repeat):
    """Reads over an indel that one haplotype carries, against the OTHER haplotype; the indel at every tenth of the read and at its midpoint.
    Yields (haplotype, read, idx0)."""
    for L in READ_LENS:
        for n in range(1, 21):
            for tenth in (1, 2, 3, 4, 5, 6, 7, 8, 9, None):
                cut = L // 2 if tenth is None else L * tenth // 10
                sign = 1 if rng.random() < 0.5 else -1
                hap_len = int(rng.integers(max(200, L + 60), 1201))
                at = int(rng.integers(L + 20, hap_len - L - 20)) if hap_len > 2 * L + 60 else hap_len // 2
                ref, alt = indel_pair(rng, hap_len, at, sign * n, int(rng.integers(1, 7)) if repeat else 0)
                off = max(at - cut, 0)                               # the read starts here in BOTH (left of the site)
                if rng.random() < 0.5:
                    src, hap = alt, ref
                else:
                    src, hap = ref, alt
                if off + L > len(src) or len(hap) < L + 15:
                    continue
                yield Hap(hap), substitute(rng, src[off:off + L]), min(off, len(hap) - L - 15)


def downstream_cases(rng, count):
    """Reads wholly right of an indel their haplotype carries: the true diagonal is idx0 + n."""
    for _ in range(count):
        L = int(rng.choice(READ_LENS))
        n = int(rng.integers(1, 21)) * (1 if rng.random() < 0.5 else -1)
        hap_len = int(rng.integers(max(200, 2 * L + 80), 1201))
        at = int(rng.integers(20, hap_len - L - 60))
        ref, alt = indel_pair(rng, hap_len, at, n)
        off = int(rng.integers(at + max(n, 0) + 1, len(alt) - L - 15))
        yield Hap(alt), substitute(rng, alt[off:off + L]), min(off - n, len(alt) - L - 15)


def edge_cases(rng, count):
    """idx0 below NBR (some neighbours are negative, some reads start left of the haplotype: idx0 < 0) and reads whose mapping position is
    clipped to the haplotype's end (they hang past it)."""
    for k in range(count):
        L = int(rng.choice(READ_LENS))
        hap_len = int(rng.integers(max(200, L + 40), 900))
        n = int(rng.integers(1, 21)) * (1 if rng.random() < 0.5 else -1)
        if k % 2 == 0:
            at = int(rng.integers(8, L))
            ref, alt = indel_pair(rng, hap_len, at, n, int(rng.integers(0, 4)))
            off = int(rng.integers(0, NBR))
            src, hap = (alt, ref) if rng.random() < 0.5 else (ref, alt)
            if off + L > len(src) or len(hap) < L + 15:
                continue
            yield Hap(hap), substitute(rng, src[off:off + L]), off - int(rng.choice([0, 0, 3, 25]))
        else:
            ref = rnd(rng, hap_len)
            off = hap_len - L - int(rng.integers(0, 15))             # right of hap_len - L - 15
            read = ref[off:off + L] + rnd(rng, L - len(ref[off:off + L]))
            yield Hap(ref), substitute(rng, read), min(off, hap_len - L - 15)


def run_cases(cases):
    res = []
    for hap, read, idx0 in cases:
        truth = unique_argmax(vote(hap, read))
        res.append((truth, old_rule(hap, read, idx0), new_rule(hap, read, idx0)[0], new_rule(hap, read, idx0, 16)[0]))
    return res


def check_sound_and_lossless(res):
    for truth, old, new, new16 in res:
        assert new is None or new == truth                          # soundness: a proven diagonal is the vote's one arg-max
        assert new16 is None or new16 == truth
        assert old is None or old == truth
        assert old is None or new == old                            # nothing the former rule proves is lost


def test_random_reference_spanning_reads():
    """Soundness, no loss, and coverage: the rule decides at least 95 % of the spanning pairs on a random reference, the former rule under 35 %.
    This file's cases (1 389 pairs, seed 1): the rule decides 1 364 (98.2 %), the former rule 366 (26.3 %); 23 pairs are ties of the vote.  With
    NBR = 16 it decides 1 260 (90.7 %): indels of 17..20 bases whose larger part lies right of the site are out of reach.  Without the count of
    read k-mers absent from the haplotype it decides 1 288 (92.7 %): a read of 36 or 50 bases with a long insertion has too few k-mers left on
    its two diagonals for the planes alone."""
    res = run_cases(spanning_cases(np.random.default_rng(1), repeat=False))
    assert len(res) >= 1300
    check_sound_and_lossless(res)
    n = len(res)
    new, old, n16 = sum(r[2] is not None for r in res), sum(r[1] is not None for r in res), sum(r[3] is not None for r in res)
    ties = sum(r[0] is None for r in res)
    print("spanning, random reference: %d pairs, new rule decides %d (NBR 16: %d), former rule %d, true ties %d" % (n, new, n16, old, ties))
    assert new >= 0.95 * n
    assert old < 0.35 * n


def test_repeats_at_the_indel():
    """Homopolymers and tandem repeats of unit 1..6 at the site: many diagonals count alike.  Soundness and no loss; what stays open goes to the
    index, hypothesis B and the queue as before."""
    res = run_cases(spanning_cases(np.random.default_rng(2), repeat=True))
    assert len(res) >= 1300
    check_sound_and_lossless(res)
    assert sum(r[0] is None for r in res) > 10                      # the vote's ties are in the batch
    assert sum(r[2] is not None for r in res) > sum(r[1] is not None for r in res)


def test_downstream_reads_and_the_edges_of_the_haplotype():
    rng = np.random.default_rng(3)
    down = run_cases(downstream_cases(rng, 300))
    check_sound_and_lossless(down)
    assert sum(r[2] is not None for r in down) >= 0.95 * len(down)
    edge = list(edge_cases(rng, 400))
    assert sum(1 for _, _, i in edge if i < 0) > 10 and sum(1 for _, _, i in edge if 0 <= i < NBR) > 50
    assert sum(1 for h, r, i in edge if i == h.n - len(r) - 15) > 50
    check_sound_and_lossless(run_cases(edge))


def test_the_neighbour_count_matches_the_kernel():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "platypus_amd", "csrc", "plat_align.hip")) as fh:
        assert "constexpr int SEED_NBR = %d;" % NBR in fh.read()


def test_the_one_diagonal_switch_parses(tmp_path):
    """tests/seed_switch_driver.cpp (a stand-alone program over csrc/switches.hpp alone, built with -fsanitize=address,undefined): PLAT_SEED_ONE_DIAG is
    on when its value begins with '1', moves no other field of AlignSwitches, and no other variable moves it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "seed_switch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-I", os.path.join(root, "platypus_amd", "csrc"), os.path.join(root, "tests", "seed_switch_driver.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        head, fields = line.split(": ")
        got[tuple(head.split(" "))] = {k: int(v) for k, v in (f.split("=") for f in fields.split())}
    rest = dict(noUngapped=0, noExact=0, noNlow=0, ungappedBigq=0, seedXcd=1, slowGroup=8, slowWaves=4, slowTiming=0, seedDebug=0, dpGridPerCu=8)
    on = {"unset": 0, "empty": 0, "0": 0, "1": 1, "yes": 0, "7": 0, "-3": 0, "10": 1, "1x": 1, "01": 0, "true": 0}
    assert got == dict([(("PLAT_SEED_ONE_DIAG", s), dict(rest, seedOneDiag=v)) for s, v in on.items()] +
                       [(("OTHERS", "1"), dict(noUngapped=1, noExact=1, noNlow=1, ungappedBigq=1, seedXcd=1, slowGroup=1, slowWaves=1, slowTiming=1,
                                               seedDebug=0, dpGridPerCu=1, seedOneDiag=0))])
