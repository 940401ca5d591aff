// refcov_driver.cpp -- a stand-alone program over platypus_amd/csrc/refcov_rule.hpp alone (tests/test_refcall_coverage_cpu.py), built with
// -fsanitize=address,undefined: the rule (count_at) against the naive loop of countReadsCoveringRegion (cwindow.pyx:176-206), and the tile
// decomposition the kernel runs -- tile_range, then count_in on a STAGED COPY of pos[iLo, iHi) / end[iLo, iHi] in heap blocks of exactly
// that size, so that an index outside the staged range is an AddressSanitizer error -- against count_at.  Seeded; prints one line per
// family, "<name> <slices> <positions>", and "ok".
#include "refcov_rule.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 11); }
static int rnd(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

// the reference's loop, written out: bisect_left twice, the walk WITHOUT the early stop, the difference
static int64_t naive(const int32_t* pos, const int32_t* end, int N, int longest, int p) {
    if (N == 0) return 0;
    const int64_t k0 = std::max<int64_t>(1, (int64_t)p - longest), k1 = (int64_t)p + 1;
    int s = 0, e = 0;
    while (s < N && pos[s] < k0) ++s;
    while (e < N && pos[e] < k1) ++e;
    while (s < N && end[s] <= p) ++s;
    return (int64_t)e - s;
}

static long check_slice(const std::vector<int32_t>& vp, const std::vector<int32_t>& ve, int longest, int from, int to, int tile) {
    const int N = (int)vp.size();
    // exact-size heap blocks: the sanitizer sees every index outside the slice
    int32_t* pos = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(N, 1));
    int32_t* end = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(N, 1));
    if (N) { memcpy(pos, vp.data(), sizeof(int32_t) * (size_t)N); memcpy(end, ve.data(), sizeof(int32_t) * (size_t)N); }
    long n = 0;
    for (int64_t a64 = from; a64 < to; a64 += tile) {
        const int a = (int)a64, b = (int)std::min<int64_t>(to, a64 + tile);
        int iLo = 0, iHi = 0;
        int32_t* sp = nullptr;
        int32_t* se = nullptr;
        if (N > 0) {
            refcov::tile_range(pos, N, longest, a, b, &iLo, &iHi);
            if (iLo < 0 || iHi < iLo || iHi > N) { printf("tile_range [%d, %d) -> [%d, %d] of %d\n", a, b, iLo, iHi, N); exit(1); }
            const int m = iHi - iLo, mEnd = m + (iHi < N ? 1 : 0);
            sp = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(m, 1));
            se = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(mEnd, 1));
            if (m) memcpy(sp, pos + iLo, sizeof(int32_t) * (size_t)m);
            if (mEnd) memcpy(se, end + iLo, sizeof(int32_t) * (size_t)mEnd);
        }
        for (int p = a; p < b; ++p, ++n) {
            const int64_t want = naive(pos, end, N, longest, p);
            const int32_t whole = refcov::count_at(pos, end, N, longest, p);
            const int32_t staged = N > 0 ? refcov::count_in(sp, se, iLo, iLo, iHi, N, longest, p) : 0;
            const bool okWhole = want < 0 ? whole < 0 : whole == want, okStaged = want < 0 ? staged < 0 : staged == want;
            if (!okWhole || !okStaged || refcov::canonical(whole) != refcov::canonical(staged)) {
                printf("p %d of tile [%d, %d), N %d longest %d: naive %lld, count_at %d, staged %d (range [%d, %d])\n", p, a, b, N, longest, (long long)want, whole, staged, iLo, iHi);
                exit(1);
            }
        }
        free(sp); free(se);
    }
    free(pos); free(end);
    return n;
}

int main() {
    long slices = 0, positions = 0;
    // ordinary tables: sorted starts, lengths 1 - 300, `longest` the table's own
    for (int it = 0; it < 300; ++it) {
        const int N = rnd(0, 400), span = rnd(1, 3000);
        std::vector<int32_t> vp((size_t)N), ve((size_t)N);
        for (int i = 0; i < N; ++i) vp[(size_t)i] = rnd(0, span);
        std::sort(vp.begin(), vp.end());
        int longest = 0;
        for (int i = 0; i < N; ++i) { const int len = rnd(1, 300); ve[(size_t)i] = vp[(size_t)i] + len; longest = std::max(longest, len); }
        positions += check_slice(vp, ve, longest, -5, span + 320, rnd(1, 1100));
        ++slices;
    }
    printf("ordinary %ld %ld\n", slices, positions);
    // odd tables: `longest` larger or smaller than the reads (also negative), reads at position 0, malformed reads (end <= pos), tiny tiles
    long s2 = 0, p2 = 0;
    for (int it = 0; it < 300; ++it) {
        const int N = rnd(1, 120), span = rnd(1, 600);
        std::vector<int32_t> vp((size_t)N), ve((size_t)N);
        for (int i = 0; i < N; ++i) vp[(size_t)i] = rnd(0, 3) == 0 ? 0 : rnd(0, span);
        std::sort(vp.begin(), vp.end());
        for (int i = 0; i < N; ++i) ve[(size_t)i] = vp[(size_t)i] + (rnd(0, 9) == 0 ? -rnd(0, 40) : rnd(1, 200));
        const int longest = rnd(0, 4) == 0 ? -rnd(0, 50) : rnd(0, 500);
        p2 += check_slice(vp, ve, longest, -30, span + 250, rnd(1, 64));
        ++s2;
    }
    printf("odd %ld %ld\n", s2, p2);
    // the ends of the number range: keys are computed in 64 bits
    {
        std::vector<int32_t> vp{1, 5, 2147483000, 2147483600}, ve{100, 2147483647, 2147483647, 2147483647};
        long n = check_slice(vp, ve, 2147483647, 2147483000, 2147483647, 1024);
        n += check_slice(vp, ve, -2147483647, -2147483647 - 1, -2147483647 + 700, 256);
        printf("extremes 2 %ld\n", n);
    }
    printf("ok\n");
    return 0;
}
