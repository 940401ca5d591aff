// source_rule.hpp -- one data line of a source VCF -> candidate alleles (plat_source_variants_batch, include/platypus_mi355x.h has the rule in
// words): variantutils.VariantCandidateReader.Variants (src/python/variantutils.py:72-159), isValidVcfLine (:168-197) and the tabix
// proxy's pos = atoi(POS) - 1 (TabProxies.pyx:608).  Plain C++ without a library, compiled for the device (plat_sourcevcf.hip) and for the
// host (host/source_variants.hpp: the host parser; tests/source_parse_driver.cpp runs it under the sanitizers).  Everything that indexes
// the text from the text's own bytes is in this file: every loop is bounded by `end`, the end of the line's region.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SRC_FN __host__ __device__ __forceinline__
#else
#define SRC_FN inline
#endif

namespace srcrule {

enum { LINE_OK = 0, LINE_SKIPPED = 1, LINE_INVALID = 2, LINE_BAD = 3 };

SRC_FN bool is_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

// hash(str) of CPython 2.7 (stringobject.c, 64-bit build), as the unsigned value
SRC_FN uint64_t py2_string_hash(const uint8_t* p, int64_t n) {
    if (n == 0) return 0;
    uint64_t x = (uint64_t)p[0] << 7;
    for (int64_t i = 0; i < n; ++i) x = (1000003ull * x) ^ p[i];
    x ^= (uint64_t)n;
    return x == ~0ull ? ~0ull - 1 : x;
}
// hash(Variant) = hash((refName, refPos, removed, added)) (tupleobject.c) narrowed to the C int of variant.pxd:31, -1 -> -2
// (the same value as py2_variant_hash of host/records.hpp, low 32 bits)
SRC_FN int32_t py2_variant_hash32(uint64_t nameHash, int32_t refPos, const uint8_t* rem, int64_t nrem, const uint8_t* add, int64_t nadd) {
    const uint64_t h[4] = {nameHash, (uint64_t)(int64_t)(refPos == -1 ? -2 : refPos), py2_string_hash(rem, nrem), py2_string_hash(add, nadd)};
    uint64_t x = 0x345678ull, mult = 1000003ull;
    for (int i = 0; i < 4; ++i) { x = (x ^ h[i]) * mult; mult += (uint64_t)(82520ll + 2 * (3 - i)); }
    x += 97531ull;
    if (x == ~0ull) x = ~0ull - 1;
    const int32_t narrowed = (int32_t)(uint32_t)x;
    return narrowed == -1 ? -2 : narrowed;
}

struct LineResult {
    int verdict;            // LINE_*
    int32_t emitted;        // alleles handed to emit (LINE_OK only)
    int32_t oversize;       // ALT elements skipped for |lenAlt - lenRef| > maxSize (LINE_OK only)
};

// The line that starts at text[a]; `end` is the end of its region's bytes (a < end).  emit(pos, rem_off, n_rem, add_off, n_add) is
// called once per allele, in ALT order, with offsets into `text`; nothing is emitted unless the verdict is LINE_OK.
template <class Emit>
SRC_FN LineResult parse_line(const uint8_t* text, int64_t a, int64_t end, int32_t maxSize, int32_t longHaps, Emit&& emit) {
    LineResult r = {LINE_SKIPPED, 0, 0};
    const uint8_t first = text[a];
    if (first == '\n' || first == '#') return r;
    // the four tabs in front of ALT, and ALT's end: a tab, the newline or the end of the region.  Nothing behind it is read
    int64_t tab[4];
    int nTab = 0;
    int64_t p = a;
    for (; p < end && nTab < 4; ++p) {
        const uint8_t c = text[p];
        if (c == '\n') break;
        if (c == '\t') tab[nTab++] = p;
    }
    r.verdict = LINE_BAD;
    if (nTab < 4) return r;                                              // fewer than five columns (where pysam raises)
    const int64_t refAt = tab[2] + 1, lenRef = tab[3] - refAt, altAt = tab[3] + 1;
    // POS: 1-10 decimal digits, at most 2^31 - 1 (beyond that atoi is undefined)
    const int64_t posAt = tab[0] + 1, nPos = tab[1] - posAt;
    if (nPos < 1 || nPos > 10) return r;
    int64_t POS = 0;
    for (int64_t i = 0; i < nPos; ++i) {
        const uint8_t c = text[posAt + i];
        if (c < '0' || c > '9') return r;
        POS = POS * 10 + (c - '0');
    }
    if (POS > 2147483647ll) return r;
    if (POS - 1 + lenRef > 2147483647ll) return r;                       // (a trimmed position would leave the C int of Variant.refPos)
    r.verdict = LINE_INVALID;
    const int64_t pos = POS - 1;
    if (pos < 0) return r;                                               // isValidVcfLine: int(position) < 0
    for (int64_t i = 0; i < lenRef; ++i) if (!is_base(text[refAt + i])) return r;
    int64_t altEnd = altAt;
    for (; altEnd < end; ++altEnd) {
        const uint8_t c = text[altEnd];
        if (c == '\t' || c == '\n') break;
        if (c != ',' && !is_base(c)) return r;
    }
    r.verdict = LINE_OK;
    for (int64_t s = altAt;;) {                                          // alts = altCol.split(","): an empty ALT is one empty element
        int64_t e = s;
        while (e < altEnd && text[e] != ',') ++e;
        const int64_t lenAlt = e - s;
        const int64_t diff = lenAlt > lenRef ? lenAlt - lenRef : lenRef - lenAlt;
        if (diff > maxSize) ++r.oversize;
        else {
            if (lenRef == 1 && lenAlt == 1) emit((int32_t)pos, refAt, (int32_t)1, s, (int32_t)1);
            else if (lenRef == lenAlt) {                                 // MNP: equal leading bases off (pos advances), then equal trailing bases
                int64_t i = 0, n = lenRef;
                while (i < lenRef && text[refAt + i] == text[s + i]) ++i;
                n -= i;
                while (n > 0 && text[refAt + i + n - 1] == text[s + i + n - 1]) --n;
                emit((int32_t)(pos + i), refAt + i, (int32_t)n, s + i, (int32_t)n);
            } else if (longHaps == 1) emit((int32_t)pos, refAt, (int32_t)lenRef, s, (int32_t)lenAlt);
            else {                                                       // ref[1:], alt[1:] (an empty one stays empty), then equal leading bases off
                const int64_t r0 = lenRef > 0 ? 1 : 0, a0 = lenAlt > 0 ? 1 : 0;
                int64_t i = 0;
                while (r0 + i < lenRef && a0 + i < lenAlt && text[refAt + r0 + i] == text[s + a0 + i]) ++i;
                emit((int32_t)(pos + i), refAt + r0 + i, (int32_t)(lenRef - r0 - i), s + a0 + i, (int32_t)(lenAlt - a0 - i));
            }
            ++r.emitted;
        }
        if (e >= altEnd) break;
        s = e + 1;
    }
    return r;
}

struct NoEmit {
    SRC_FN void operator()(int32_t, int64_t, int32_t, int64_t, int32_t) const {}
};

}  // namespace srcrule
