// fasta_rule.hpp -- the rule of the indexed FASTA fetch (plat_fasta_fetch_batch, include/platypus_mi355x.h has it in words): what
// FastaIndex.getRefs (src/cython/fastafile.pyx:64-82), FastaFile.getCharacter (:120-139) and FastaFile.getSequence (:173-207, the same
// arithmetic as setCacheSequence :141-171) do, restated.  Plain C++ without a library, compiled for the device (plat_fasta.hip) and for the
// host (host/fasta_source.hpp: the host twin and the .fai parse; tests/fasta_host_driver.cpp runs it under the sanitizers).  One statement
// of each piece: the file offset of a base (offset_of), the span of one query and the way the call ends (span_of), the bytes a span gives
// (keeps, upper), the cut of a span at the uploaded bytes (cut_of) and one line of a .fai (parse_fai_line).
//
// The reference never looks at the bytes it seeks over: a base's offset is line arithmetic on the index's numbers alone, so an index that
// lies (a ragged middle line, a wrong LineLength) reads whatever lies there -- header bytes included.  That is kept.  The quotient
// pos / LineLength is taken in fp64 and truncated, as the reference takes it (exact below 2^53, and the same rounding above).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FASTA_FN __host__ __device__ __forceinline__
#else
#define FASTA_FN inline
#endif

namespace fasta {

// how a query ends (plat_fasta_fetch_batch's out_status, PLAT_FASTA_*)
constexpr int32_t ST_OK = 0;                                               // bytes (possibly none)
constexpr int32_t ST_INDEX_ERROR = 1;                                      // IndexError: "Cannot have beginPos = %s, endPos = %s" (end < beg after the clamps)
constexpr int32_t ST_ZERO_LINE = 2;                                        // LineLength == 0: the reference divides by it
constexpr int32_t ST_BAD_INDEX = 3;                                        // StartPos < 0, LineLength < 0 or FullLineLength < LineLength: lines plat_fasta_open refuses
constexpr int32_t ST_LEFT_OF_CUT = 4;                                      // the span begins in front of the uploaded bytes
constexpr int32_t ST_RIGHT_OF_CUT = 5;                                     // the span ends behind the uploaded bytes

constexpr uint8_t MODE_SEQUENCE = 0;                                       // getSequence(beg, end): never the contig's last base
constexpr uint8_t MODE_CONTIG = 1;                                         // all SeqLength bases; beg and end are not read

struct Entry { int64_t start_pos, line_len, full_len, seq_len; };          // one .fai line's numbers
struct Span { int64_t lo, hi; int32_t status; };                           // file offsets [lo, hi), lo <= hi; both 0 unless status is ST_OK

// the file offset of base `pos` (line_len != 0).  Sums wrap in 64 bits instead of overflowing: whatever an index claims, the result is a number
FASTA_FN int64_t offset_of(const Entry& e, int64_t pos)
{
    const int64_t lines = (int64_t)((double)pos / (double)e.line_len);
    return (int64_t)((uint64_t)e.start_pos + (uint64_t)pos + (uint64_t)(e.full_len - e.line_len) * (uint64_t)lines);
}

// the entry's numbers are ones the line arithmetic can run on
FASTA_FN int32_t entry_status(const Entry& e)
{
    if (e.line_len == 0) return ST_ZERO_LINE;
    if (e.start_pos < 0 || e.line_len < 0 || e.full_len < e.line_len) return ST_BAD_INDEX;
    return ST_OK;
}

// the span of one query in a file of file_size bytes.  The reference computes both offsets (and divides) before it compares beg and end,
// so a zero LineLength ends the call whatever the positions are.
FASTA_FN Span span_of(const Entry& e, int64_t beg, int64_t end, uint8_t mode, int64_t file_size)
{
    const int32_t es = entry_status(e);
    if (es != ST_OK) return Span{0, 0, es};
    int64_t b, last;
    if (mode == MODE_CONTIG) {
        if (e.seq_len <= 0) return Span{0, 0, ST_OK};
        b = 0; last = e.seq_len - 1;
    } else {
        b = beg < 0 ? 0 : beg;
        last = e.seq_len - 1 < end ? e.seq_len - 1 : end;
        if (last < b) return Span{0, 0, ST_INDEX_ERROR};
    }
    int64_t lo = offset_of(e, b), hi = offset_of(e, last);
    if (mode == MODE_CONTIG) hi = (int64_t)((uint64_t)hi + 1u);               // ... through the last base
    if (lo < 0 || hi < lo) return Span{0, 0, ST_BAD_INDEX};                   // (sums that wrapped)
    if (lo > file_size) lo = file_size;                                       // a seek past the end reads nothing
    if (hi > file_size) hi = file_size;
    return Span{lo, hi, ST_OK};
}

// the span against the cut [file_base, file_base + file_len) of the file that was uploaded; an empty span lies inside every cut
FASTA_FN int32_t cut_of(const Span& s, int64_t file_base, int64_t file_len)
{
    if (s.status != ST_OK || s.lo >= s.hi) return s.status;
    if (s.lo < file_base) return ST_LEFT_OF_CUT;
    if (s.hi - file_base > file_len) return ST_RIGHT_OF_CUT;
    return ST_OK;
}

// replace("\n", "").upper(): 0x0A goes, a-z become A-Z, every other byte -- '\r', NUL, bytes >= 0x80 -- stays
FASTA_FN bool keeps(uint8_t c) { return c != 0x0A; }
FASTA_FN uint8_t upper(uint8_t c) { return (uint8_t)(c - 'a') < 26u ? (uint8_t)(c & 0xDFu) : c; }
// ... four bytes at once: the bytes of w that are a-z, as 0x20 each (the high bits of the two sums say >= 'a' and > 'z'; bytes >= 0x80 are left out)
FASTA_FN uint32_t upper4(uint32_t w)
{
    const uint32_t t = w & 0x7f7f7f7fu;
    const uint32_t lower = (t + 0x1f1f1f1fu) & ~(t + 0x05050505u) & ~w & 0x80808080u;
    return w ^ (lower >> 2);
}

// getCharacter(pos): the byte at base pos's offset, upper-cased; '-' outside [0, SeqLength); -1 where the file ends in front of the offset
// (the reference's read(1) returns an empty string there).  *status: ST_OK, or the entry's status when pos lies inside the contig
FASTA_FN int character_at(const Entry& e, int64_t pos, const uint8_t* file, int64_t file_size, int32_t* status)
{
    *status = ST_OK;
    if (pos >= e.seq_len || pos < 0) return '-';
    if ((*status = entry_status(e)) != ST_OK) return '-';
    const int64_t at = offset_of(e, pos);
    if (at < 0) { *status = ST_BAD_INDEX; return '-'; }
    return at < file_size ? (int)upper(file[at]) : -1;
}

// ---- one line of a .fai -----------------------------------------------------------------------------------------------
FASTA_FN bool is_space(uint8_t c) { return c == ' ' || (c >= 0x09 && c <= 0x0D); }     // what str.strip() and str.split() take for white space

// atoll: white space, a sign, digits; whatever follows is not read.  Saturates as strtoll does
FASTA_FN int64_t atoll_of(const uint8_t* s, int64_t n)
{
    int64_t i = 0;
    while (i < n && is_space(s[i])) ++i;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; ++i; }
    uint64_t v = 0;
    const uint64_t limit = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
    for (; i < n && s[i] >= '0' && s[i] <= '9'; ++i) {
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (v > (limit - d) / 10) { v = limit; while (i < n && s[i] >= '0' && s[i] <= '9') ++i; break; }
        v = v * 10 + d;
    }
    return neg ? (int64_t)(0 - v) : (int64_t)v;
}

constexpr int FAI_OK = 0, FAI_FEW_FIELDS = 1, FAI_NO_NAME = 2;
struct FaiLine { int64_t name_at, name_len; Entry e; };                    // the name: bytes [name_at, name_at + name_len) of the line

// line [0, n): one line of the index as the file iterator hands it over (its '\n' may be there or not).  strip(), split on tabs, the
// name the first white-space-separated token of field 0 -- with parseNCBI a name gi|..|ref|X|.. becomes X --, fields 1 to 4 through atoll.
// The reference reads line[0].split()[0] before line[1] .. line[4]: a name field without a token comes first.
FASTA_FN int parse_fai_line(const uint8_t* line, int64_t n, int parseNCBI, FaiLine* out)
{
    int64_t a = 0, b = n;
    while (a < b && is_space(line[a])) ++a;
    while (b > a && is_space(line[b - 1])) --b;
    int64_t at[6];                                                          // the first five fields' starts, and the end of the fifth
    int fields = 0;
    at[0] = a;
    for (int64_t i = a; i <= b && fields < 5; ++i)
        if (i == b || line[i] == '\t') at[++fields] = i + 1;
    // (fields: how many of the first five are there; field k is [at[k], at[k + 1] - 1))
    int64_t n0 = at[0], n1 = fields >= 1 ? at[1] - 1 : b;
    while (n0 < n1 && is_space(line[n0])) ++n0;
    int64_t ne = n0;
    while (ne < n1 && !is_space(line[ne])) ++ne;
    if (ne == n0) return FAI_NO_NAME;
    if (fields < 5) return FAI_FEW_FIELDS;
    if (parseNCBI && ne - n0 >= 3 && line[n0] == 'g' && line[n0 + 1] == 'i' && line[n0 + 2] == '|') {
        int64_t bar[4], bars = 0;                                           // the first four '|': parts 0 .. 3 lie between them
        for (int64_t i = n0; i < ne && bars < 4; ++i) if (line[i] == '|') bar[bars++] = i;
        if (bars >= 3 && bar[2] - bar[1] == 4 && line[bar[1] + 1] == 'r' && line[bar[1] + 2] == 'e' && line[bar[1] + 3] == 'f') {
            n0 = bar[2] + 1;
            if (bars == 4) ne = bar[3];
        }
    }
    out->name_at = n0; out->name_len = ne - n0;
    int64_t v[4];
    for (int k = 0; k < 4; ++k) v[k] = atoll_of(line + at[k + 1], at[k + 2] - 1 - at[k + 1]);
    out->e.seq_len = v[0]; out->e.start_pos = v[1]; out->e.line_len = v[2]; out->e.full_len = v[3];
    return FAI_OK;
}

}  // namespace fasta
