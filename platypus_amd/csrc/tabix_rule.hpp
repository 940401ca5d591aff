// tabix_rule.hpp -- one line of a tabix fetch over a bgzipped VCF (plat_tabix_fetch_batch, include/platypus_mi355x.h has the rule in words):
// ti_iter_read (src/tabix/index.c.pysam.c:872-911), ti_get_intv with the VCF preset (:161-225) and get_intv (:227-241).  Plain C++ without a
// library, compiled for the device (plat_tabix.hip) and for the host (host/tabix_source.hpp: the host path; tests/tabix_host_driver.cpp runs
// it under the sanitizers).  Everything that indexes the text from the text's own bytes is in this file: every loop is bounded by the
// line's end, which its caller bounds by the chunk's bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TBX_FN __host__ __device__ __forceinline__
#else
#define TBX_FN inline
#endif

namespace tbxrule {

enum { LINE_KEEP = 0, LINE_SKIP = 1, LINE_STOP = 2, LINE_REFUSE = 3 };
constexpr int64_t INT_LIMIT = 2147483647;                  // a POS or an end beyond +-(2^31 - 1) refuses: the reference narrows a long to int32 there

TBX_FN bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
TBX_FN int digit_of(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'z' ? c - 'a' + 10 : c >= 'A' && c <= 'Z' ? c - 'A' + 10 : 99; }

// strtol(text + p, , 0) for a string that ends at `limit` (where the reference's has its NUL): leading C white space, an optional sign,
// 0x / 0X hex (when a hex digit follows), a leading 0 octal, otherwise decimal; stops at the first byte that is no digit of the base; no
// digits gives 0.  *wide: the value lies outside +-INT_LIMIT (it is then clamped to INT_LIMIT + 1 in size).
TBX_FN int64_t strtol0(const uint8_t* text, int64_t p, int64_t limit, bool* wide) {
    while (p < limit && is_space(text[p])) ++p;
    bool neg = false;
    if (p < limit && (text[p] == '+' || text[p] == '-')) { neg = text[p] == '-'; ++p; }
    int base = 10;
    if (p < limit && text[p] == '0') {
        if (p + 2 < limit && (text[p + 1] == 'x' || text[p + 1] == 'X') && digit_of(text[p + 2]) < 16) { base = 16; p += 2; }
        else base = 8;
    }
    int64_t v = 0;
    for (; p < limit; ++p) {
        const int d = digit_of(text[p]);
        if (d >= base) break;
        if (v <= INT_LIMIT) v = v * base + d;                              // (at most 36 * 2^31: no overflow; beyond the limit it stays there)
    }
    if (v > INT_LIMIT) { *wide = true; v = INT_LIMIT + 1; }
    return neg ? -v : v;
}

// the first occurrence of pat[0 .. n) in text[a, b), or -1
TBX_FN int64_t find_in(const uint8_t* text, int64_t a, int64_t b, const char* pat, int n) {
    for (int64_t p = a; p + n <= b; ++p) {
        int k = 0;
        while (k < n && text[p + k] == (uint8_t)pat[k]) ++k;
        if (k == n) return p;
    }
    return -1;
}

// The verdict of the line text[s, e) (e: its '\n' or the end of its chunk's bytes) for the fetch of sequence name[0 .. nameLen) over
// [beg, end).  Columns 1 to 8 are read and nothing behind the tab that ends column 8.
TBX_FN int line_verdict(const uint8_t* text, int64_t s, int64_t e, const uint8_t* name, int32_t nameLen, int32_t beg, int32_t end) {
    if (s < e && text[s] == '#') return LINE_SKIP;                         // (the meta character of the VCF preset)
    int id = 1;
    bool sameName = false, wide = false;
    int64_t b = 0, en = -1;                                                // the interval, 0-based half-open
    int64_t colAt = s;
    for (int64_t i = s; i <= e && id <= 8; ++i) {
        if (i < e && text[i] != '\t' && text[i] != 0) continue;
        if (id == 1) {
            sameName = i - colAt == nameLen;
            for (int32_t k = 0; sameName && k < nameLen; ++k) sameName = text[colAt + k] == name[k];
        } else if (id == 2) {
            // (as the reference's strtol, this one runs on from the column's start to the line's end: white space -- a tab is some -- in
            //  front of the number is passed over wherever it stands)
            const int64_t v = strtol0(text, colAt, e, &wide);
            b = v - 1 < 0 ? 0 : v - 1;
            en = v < 1 ? 1 : v;
        } else if (id == 4) {
            if (colAt < i) en = b + (i - colAt);
        } else if (id == 8) {
            int64_t at = find_in(text, colAt, i, "END=", 4);
            if (at == colAt) at += 4;
            else if (at >= 0) { at = find_in(text, colAt, i, ";END=", 5); if (at >= 0) at += 5; }
            if (at >= 0) en = strtol0(text, at, i, &wide);
        }
        colAt = i + 1;
        ++id;
    }
    if (id <= 2) return LINE_STOP;                                         // fewer than two columns: no interval, the reference's tid -1
    if (wide || en > INT_LIMIT) return LINE_REFUSE;
    if (en < 0 || !sameName || b >= end) return LINE_STOP;
    return en > beg && end > b ? LINE_KEEP : LINE_SKIP;
}

// One stream walked on the host, chunk by chunk, over bytes that lie as plat_bgzf_inflate_batch leaves them.  Chunk q of nChunks is
// text[lo[q], hi[q]), its first line starts at first[q] and it ends at stop[q] (lo <= stop <= hi).  emit(lineStart, lineEnd) is called for
// every kept line; walked / kept count the lines ahead of the stop.  Returns false when the stream is refused.
template <class Emit>
inline bool walk_stream(const uint8_t* text, int nChunks, const int64_t* first, const int64_t* stop, const int64_t* hi, const uint8_t* name,
                        int32_t nameLen, int32_t beg, int32_t end, int64_t* walked, int64_t* kept, Emit&& emit) {
    *walked = 0; *kept = 0;
    for (int q = 0; q < nChunks; ++q) {
        int64_t p = first[q];
        while (p < stop[q] && p < hi[q]) {
            int64_t e = p;
            while (e < hi[q] && text[e] != '\n') ++e;
            const int v = line_verdict(text, p, e, name, nameLen, beg, end);
            if (v == LINE_REFUSE) return false;
            if (v == LINE_STOP) return true;
            ++*walked;
            if (v == LINE_KEEP) { ++*kept; emit(p, e); }
            p = e < hi[q] ? e + 1 : e;
        }
        if (q + 1 < nChunks && p > stop[q]) return false;                  // (the reference asserts curr_off == off[i].v)
    }
    return true;
}

}  // namespace tbxrule
