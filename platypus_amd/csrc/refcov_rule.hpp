// refcov_rule.hpp -- the read count a REFCALL line is built on (plat_refcall_coverage_batch, include/platypus_mi355x.h has the rule in
// words): ReadArray.countReadsCoveringRegion(p, p + 1) (cwindow.pyx:176-206) as outputRefCall loops it over a block's positions
// (variantcaller.pyx:774-784).  Plain C++ without a library, compiled for the device (plat_refcov.hip) and for the host (host/stage_f.hpp:
// refCallLine, coverageHasAZero; tests/refcov_driver.cpp runs it under the sanitizers).  One statement of the rule: the count of ONE
// position inside a range of the slice that is known to hold its two bounds (count_in), the range that holds the bounds of every position
// of a tile (tile_range), and the count over the whole slice (count_at = count_in over [0, N]).
//
// The count is a difference of two pointers, not the number of covering reads: a short read lying between two covering reads is counted,
// and a read at position 0 is never found by the first bound (its key is at least 1).  A negative count is where the reference raises
// ("Read start pointer > read end pointer"): the walk stops at the first such index and the count is returned as it stands then.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define REFCOV_FN __host__ __device__ __forceinline__
#else
#define REFCOV_FN inline
#endif

namespace refcov {

constexpr int32_t RAISES = -1;                                             // PLAT_REFCOV_RAISES: every negative count, canonicalised
constexpr int32_t EMPTY = 2147483647;                                      // PLAT_REFCOV_EMPTY: the minimum over nothing
constexpr int TILE = 1024;                                                 // positions of one tile (one workgroup)

// first index i in [lo, hi) with a[i - bias] >= key, hi if there is none; a[] ascending
REFCOV_FN int lower_bound(const int32_t* a, int bias, int lo, int hi, int64_t key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)a[mid - bias] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// [iLo, iHi] for the positions [a, b), a < b, of a slice of N > 0 reads: the two bounds of every position p of the tile lie inside it.  The keys
// of p are max(1, p - longest) and p + 1, both ascending in p, so the smallest key of the tile is the smaller key of a and the largest the
// larger key of b - 1.  For a tile at positions >= 0 and longest >= 0 that is iLo = lb(max(1, a - longest)), iHi = lb(b); the general form
// keeps a table with a negative `longest` or a block in front of position 0 exact as well.  The walk of a position reads end[] at indices
// up to its second bound, so at most at iHi -- which is a read of the slice only when iHi < N.
REFCOV_FN void tile_range(const int32_t* pos, int N, int longest, int a, int b, int* iLo, int* iHi) {
    const int64_t ka = (int64_t)a - longest < 1 ? 1 : (int64_t)a - longest, kb = (int64_t)b - 1 - longest < 1 ? 1 : (int64_t)b - 1 - longest;
    const int64_t lowest = ka < (int64_t)a + 1 ? ka : (int64_t)a + 1, highest = kb > (int64_t)b ? kb : (int64_t)b;
    *iLo = lower_bound(pos, 0, 0, N, lowest);
    *iHi = lower_bound(pos, 0, *iLo, N, highest);
}

// the count at p from pos[i - bias] / end[i - bias], i in [iLo, iHi] (end[iHi - bias] is read only when iHi < N); N > 0
REFCOV_FN int32_t count_in(const int32_t* pos, const int32_t* end, int bias, int iLo, int iHi, int N, int longest, int p) {
    const int64_t k = (int64_t)p - longest;
    int s0 = lower_bound(pos, bias, iLo, iHi, k < 1 ? 1 : k);
    const int e0 = lower_bound(pos, bias, iLo, iHi, (int64_t)p + 1);
    while (s0 <= e0 && s0 < N && end[s0 - bias] <= p) ++s0;
    return e0 - s0;
}

// ... over the whole slice; N == 0 counts nothing
REFCOV_FN int32_t count_at(const int32_t* pos, const int32_t* end, int N, int longest, int p) {
    return N > 0 ? count_in(pos, end, 0, 0, N, N, longest, p) : 0;
}

REFCOV_FN int32_t canonical(int32_t c) { return c < 0 ? RAISES : c; }

}  // namespace refcov
