// mate_rule.hpp -- the rule of the broken-mate fetch (plat_bam_mates_batch, include/platypus_mi355x.h; host/bam_mates.hpp): what loadBAMData
// does with the mates of improper pairs (src/cython/platypusutils.pyx:522-559 and :617-654, mergeQueries :690-707), restated.  Plain C++
// without a library, compiled for the device (plat_bammates.hip) and for the host (host/bam_mates.hpp; tests/mate_rule_host_driver.cpp runs
// it under the sanitizers).  One statement of each piece: the fixed fields of a record wherever it lies (fields_of), which kept record gives
// a coordinate (gives_coord), which record of a second-round fetch is a broken mate (is_mate), the order of the coordinates (coord_less),
// mergeQueries (merge_queries) and the window of a query's fetch (query_window).
//
// Both branches of :525-533 append (name of mtid, mtid, mpos) unless mtid == -1: a fetched record's own refID is the fetch's tid and never
// -1, so `mateChromID == chromID` implies mtid != -1.  QC plays no part: the coordinates come from every record the iterator returned.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MATE_FN __host__ __device__ __forceinline__
#else
#define MATE_FN inline
#endif

namespace mate {

constexpr int FIXED_BYTES = 32;                                            // refID .. tlen: what a record has to hold before a field is read
constexpr int OFF_FLAG = 14, OFF_MTID = 20, OFF_MPOS = 24;                 // counted from the record's refID
constexpr int MERGE_GAP = 10000, MERGE_SPAN = 100000;                      // mergeQueries' 1e4 and 1e5

struct Fields { uint16_t flag; int32_t mtid, mpos; };
struct Coord { int32_t mtid, mpos; };
struct Query { int32_t mtid; int64_t start, end; };                        // [start, end) as mergeQueries leaves them (end may be 2^31); mtid: the coordinate that opened it

// flag, next_refID and next_pos of the record whose refID is rec[0]; Bytes: anything with operator[] over uint8_t (records lie at any alignment)
template <class Bytes> MATE_FN Fields fields_of(const Bytes& rec)
{
    auto u32 = [&](int at) { return (uint32_t)rec[at] | ((uint32_t)rec[at + 1] << 8) | ((uint32_t)rec[at + 2] << 16) | ((uint32_t)rec[at + 3] << 24); };
    Fields f;
    f.flag = (uint16_t)((uint32_t)rec[OFF_FLAG] | ((uint32_t)rec[OFF_FLAG + 1] << 8));
    f.mtid = (int32_t)u32(OFF_MTID);
    f.mpos = (int32_t)u32(OFF_MPOS);
    return f;
}

// (not Read_IsProperPair) or Read_IsUnmapped or Read_MateIsUnmapped, and a mate contig to look on
MATE_FN bool gives_coord(const Fields& f) { return (!(f.flag & 0x2) || (f.flag & 0x4) || (f.flag & 0x8)) && f.mtid != -1; }

// :556 / :647 -- mtid == chromID and start <= mpos <= end, both ends inclusive, with loadBAMData's arguments
MATE_FN bool is_mate(const Fields& f, int32_t region_tid, int32_t start, int32_t end) { return f.mtid == region_tid && start <= f.mpos && f.mpos <= end; }

// the order list.sort() gives (name, mtid, mpos) tuples: name_cmp(a.mtid, b.mtid) compares the contigs' names bytewise (< 0, 0, > 0)
template <class NameCmp> inline bool coord_less(const Coord& a, const Coord& b, NameCmp&& name_cmp)
{
    const int c = a.mtid == b.mtid ? 0 : name_cmp(a.mtid, b.mtid);
    if (c != 0) return c < 0;
    if (a.mtid != b.mtid) return a.mtid < b.mtid;
    return a.mpos < b.mpos;
}

// mergeQueries over n sorted coordinates: emit(Query) for every query, in order.  same_name(a, b): the contigs of two mtids have equal names
template <class SameName, class Emit> inline void merge_queries(const Coord* coords, long long n, SameName&& same_name, Emit&& emit)
{
    Query q{0, 0, 0};
    bool open = false;
    for (long long i = 0; i < n; ++i) {
        const Coord& c = coords[i];
        if (open && same_name(c.mtid, q.mtid) && (int64_t)c.mpos - q.end < MERGE_GAP && (int64_t)c.mpos - q.start < MERGE_SPAN) { q.end = (int64_t)c.mpos + 1; continue; }
        if (open) emit(q);
        q = Query{c.mtid, (int64_t)c.mpos, (int64_t)c.mpos + 1};
        open = true;
    }
    if (open) emit(q);
}

// the window of sam_itr_querys("%s:%s-%s" % (name, start, end)) (htslib's hts_parse_reg: 1-based inclusive text)
// (an end of 2^31 is held at INT32_MAX, the largest window the index query takes)
MATE_FN void query_window(const Query& q, int32_t* itr_beg, int32_t* itr_end)
{
    *itr_beg = (int32_t)(q.start - 1 > 0 ? q.start - 1 : 0);
    *itr_end = (int32_t)(q.end > 2147483647ll ? 2147483647ll : q.end);
}

}  // namespace mate
