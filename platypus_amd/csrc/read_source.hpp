// read_source.hpp -- device-only: a read's letters and qualities wherever they lie (expanded ASCII bytes or PLAT_READS_PACKED bytes at their
// source), for the kernels that start from a READ: the candidate scan on codes (plat_candidates.hip), the INFO read statistics
// (plat_infostats.hip) and the window gather (plat_readtable.hip); and the unaligned 64-bit load the byte scan and the unpack passes share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/platypus_mi355x.h"

namespace plat {

// 8 bytes from any address (global memory takes unaligned 64-bit loads)
__device__ __forceinline__ unsigned long long load_u64_bytes(const uint8_t* p) {
    typedef unsigned long long __attribute__((aligned(1))) u64u;
    return *(const u64u*)p;
}

__device__ __forceinline__ bool has_n(const uint8_t* s, int n) {
    for (int i = 0; i < n; ++i) if (s[i] == 'N') return true;
    return false;
}

// ---- a read's letters and qualities, wherever they lie ------------------------------------------------------------------------------------
// The kernels that start from a READ (the scan on codes, the read statistics, the gather) are written once over one of these: base(i) /
// qual(i) of the read's i-th base (qual: the raw byte; the scan reads it unsigned, the statistics signed, as the reference's two loops do).
// ASCII tables: the expanded bytes.
struct ReadAscii {
    const uint8_t* s; const uint8_t* q;
    __device__ __forceinline__ uint8_t base(int i) const { return s[i]; }
    __device__ __forceinline__ uint8_t qual(int i) const { return q[i]; }
    __device__ __forceinline__ bool has_n(int at, int n) const { return plat::has_n(s + at, n); }
};
struct SrcAscii {
    static constexpr bool packed = false;
    const uint8_t* seq; const uint8_t* qual;
    __device__ __forceinline__ ReadAscii read(int, long long soff, long long) const { return ReadAscii{seq + soff, qual + soff}; }
};
// PLAT_READS_PACKED bytes at their source: letter "ACTG"[b & 3], quality b >> 2 -- or the exception's, where the blob index at + i is listed
// in exc_index[e0, e1) (the read's own exceptions: two lower bounds per read, and only in a chunk that has any; most reads have none and
// never touch the exception arrays)
struct ReadPacked {
    const uint8_t* p; long long at; const int64_t* idx; const uint8_t* eb; const uint8_t* eq; long long e0, e1;
    __device__ __forceinline__ long long find(int i) const {
        long long lo = e0, hi = e1;
        while (lo < hi) { const long long mid = (lo + hi) >> 1; if (idx[mid] < at + i) lo = mid + 1; else hi = mid; }
        return lo < e1 && idx[lo] == at + i ? lo : -1;
    }
    __device__ __forceinline__ uint8_t base(int i) const {
        if (e0 != e1) { const long long k = find(i); if (k >= 0) return eb[k]; }
        return (uint8_t)((0x47544341u >> (8u * (p[i] & 3u))) & 0xFFu);
    }
    __device__ __forceinline__ uint8_t qual(int i) const {
        if (e0 != e1) { const long long k = find(i); if (k >= 0) return eq[k]; }
        return (uint8_t)(p[i] >> 2);
    }
    __device__ __forceinline__ bool has_n(int a, int n) const {                    // (only an exception can be an N)
        for (long long k = e0; k < e1; ++k) if (idx[k] >= at + a && idx[k] < at + a + n && eb[k] == 'N') return true;
        return false;
    }
};
struct SrcPacked {
    static constexpr bool packed = true;
    plat_packed_reads pk;
    // read r, whose bytes are [soff, soff + rlen) of the blob
    __device__ __forceinline__ ReadPacked read(int r, long long soff, long long rlen) const {
        long long e0 = 0, e1 = 0;
        if (pk.n_exc > 0) {
            long long lo = 0, hi = pk.n_exc;
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if (pk.exc_index[mid] < soff) lo = mid + 1; else hi = mid; }
            e0 = lo; hi = pk.n_exc;
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if (pk.exc_index[mid] < soff + rlen) lo = mid + 1; else hi = mid; }
            e1 = lo;
        }
        return ReadPacked{pk.read_src[r], soff, pk.exc_index, pk.exc_base, pk.exc_qual, e0, e1};
    }
};
}  // namespace plat
