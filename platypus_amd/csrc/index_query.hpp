// index_query.hpp -- the chunk list of a region query over a tabix index (.tbi) or a BAM index (.bai): ti_iter_query
// (src/tabix/index.c.pysam.c:776-870; a BAI has the same bins, so one rule serves both).  include/platypus_mi355x.h has the rule in words
// next to the device entry point, plat_index_query_batch.  Plain C++ without a library.  Three parts:
//   the rule of one query (level_range, lin_slot, the status block): compiled for the device (plat_idxquery.hip) and for the host;
//   the flatten (flatten): the index's bytes to flat tables.  The format is SERIAL -- every count moves what follows it -- so this is host
//   work, done once per file when the index is opened; the tables then live on the device and no query reads the bytes again;
//   the host twin (query) of the device call, over the same tables; resolve_serial is the reference's three loops as they stand,
//   resolve_parallel the three data-parallel steps that restate them, resolve_fused the one scan the kernels run.
// host/index_source.hpp runs the twin under PLAT_CALLER_HOST_INDEX=1 and for queries the device hands over;
// tests/index_query_host_driver.cpp builds this file alone under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IDXQ_FN __host__ __device__ __forceinline__
#else
#define IDXQ_FN inline
#endif

namespace idxq {

// the status block, in 64-bit words
enum { ST_VERDICT = 0, ST_QUERY = 1, ST_CHUNKS = 2, ST_GATHERED = 3, ST_HANDED = 4, ST_NO_ITER = 5, ST_WORDS = 6 };
constexpr int ERR_INVALID = -1, ERR_UNSUPPORTED = -6, ERR_OVERFLOW = -8, ERR_BAD_INPUT = -9;      // (PLAT_ERR_* of the same names)
constexpr int KIND_TBI = 0, KIND_BAI = 1;
constexpr int LIDX_SHIFT = 14;
constexpr int MAX_BIN = 37450;                            // the bins are 0 .. 37448; 37450 itself is the metadata pseudo-bin
constexpr int MAX_REF = 65536;                            // (PLAT_TBI_MAX_REF)
constexpr int MAX_CHUNKS = 2048;                          // (PLAT_IDXQ_MAX_CHUNKS) gathered chunks one query is answered with on the device
constexpr int COUNT_NO_ITER = -1, COUNT_HANDED = -2;
constexpr int LEVELS = 6;

// The bins of level `level` (0: bin 0 alone ... 5: the 16 kb bins) that reg2bins lists for [beg, end): lo .. hi inclusive.
// beg >= 0 and beg < end (the caller has returned for everything else); end is clamped to 2^29 and end - 1 used, as the reference does.
IDXQ_FN void level_range(int level, int32_t beg, int32_t end, int32_t* lo, int32_t* hi)
{
    const uint32_t b = (uint32_t)beg, e = ((uint32_t)end >= (1u << 29) ? (1u << 29) : (uint32_t)end) - 1u;
    if (level == 0) { *lo = 0; *hi = 0; return; }
    const int shift = 29 - 3 * level;
    const int32_t first = (int32_t)(((1u << (3 * level)) - 1u) / 7u);            // 1, 9, 73, 585, 4681
    *lo = first + (int32_t)(b >> shift); *hi = first + (int32_t)(e >> shift);
}

// the first position in ids[lo, hi) (ascending) whose id is >= want
IDXQ_FN int64_t lower_bound(const int32_t* ids, int64_t lo, int64_t hi, int32_t want)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the linear index's entry a query that begins at beg reads, or -1 for an empty linear index (min_off 0)
IDXQ_FN int64_t lin_slot(int32_t beg, int64_t n_lin) { const int64_t k = beg >> LIDX_SHIFT; return n_lin <= 0 ? -1 : k < n_lin ? k : n_lin - 1; }

IDXQ_FN bool pair_less(uint64_t ua, uint64_t va, uint64_t ub, uint64_t vb) { return ua != ub ? ua < ub : va < vb; }

}  // namespace idxq

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace idxq {

typedef std::pair<uint64_t, uint64_t> Chunk;              // (u, v) virtual offsets

// the flat tables of one index
struct Flat {
    int kind = KIND_TBI;
    int32_t nRef = 0;
    std::vector<int64_t> refBinFirst{0};                  // [nRef + 1] into binId
    std::vector<int32_t> binId;                           // ascending within a reference
    std::vector<int64_t> binChunkFirst{0};                // [bins + 1] into chunkU / chunkV
    std::vector<int64_t> chunkU, chunkV;                  // file order within a bin
    std::vector<int64_t> refLinFirst{0};                  // [nRef + 1] into linFill
    std::vector<int64_t> linFill;                         // lin[i] when non-zero, else the last non-zero entry below i, else 0
    std::vector<std::string> names;                       // a .tbi's
    int64_t noCoor = -1;                                  // a .bai's trailing n_no_coor, -1 when it has none
    void clear() { *this = Flat(); }
};

struct Reader {
    const uint8_t* p; size_t len, at = 0; bool ok = true;
    bool need(uint64_t n) { if (!ok || n > len - at) ok = false; return ok; }
    uint32_t u32() { if (!need(4)) return 0; uint32_t v = 0; for (int k = 0; k < 4; ++k) v |= (uint32_t)p[at + k] << (8 * k); at += 4; return v; }
    uint64_t u64() { if (!need(8)) return 0; uint64_t v = 0; for (int k = 0; k < 8; ++k) v |= (uint64_t)p[at + k] << (8 * k); at += 8; return v; }
};

// The index's bytes (a .tbi's after BGZF inflation) to flat tables.  0, or ERR_BAD_INPUT (the bytes end before a count says they should,
// a negative count, a bin twice in one reference, a bin id of 37450 or above that is not the pseudo-bin, a bad magic, names that are not
// n_ref NUL-ended strings inside l_nm) or ERR_UNSUPPORTED (a preset other than VCF's, more than MAX_REF references).  Every read is
// checked against len first: no input makes this read outside raw[0, len).  F is left empty when the bytes are refused.
inline int flatten(const uint8_t* raw, size_t len, int kind, Flat& F)
{
    F.clear();
    F.kind = kind;
    Reader r{raw, len};
    auto refuse = [&](int code) { F.clear(); F.kind = kind; return code; };
    if (!raw && len) return refuse(ERR_INVALID);
    if (!r.need(4) || memcmp(raw, kind == KIND_TBI ? "TBI\1" : "BAI\1", 4) != 0) return refuse(ERR_BAD_INPUT);
    r.at = 4;
    const int32_t nRef = (int32_t)r.u32();
    if (!r.ok || nRef < 0) return refuse(ERR_BAD_INPUT);
    if (nRef > MAX_REF) return refuse(ERR_UNSUPPORTED);
    if (kind == KIND_TBI) {
        int32_t w[7];                                                           // format, col_seq, col_beg, col_end, meta, skip, l_nm
        for (int k = 0; k < 7; ++k) w[k] = (int32_t)r.u32();
        if (!r.ok || w[6] < 0) return refuse(ERR_BAD_INPUT);
        if ((w[0] & 0xffff) != 2) return refuse(ERR_UNSUPPORTED);               // (TI_PRESET_VCF)
        if (!r.need((uint64_t)w[6])) return refuse(ERR_BAD_INPUT);
        size_t at = r.at;
        const size_t end = r.at + (size_t)w[6];
        for (int32_t t = 0; t < nRef; ++t) {
            const void* z = at < end ? memchr(raw + at, 0, end - at) : nullptr;
            if (!z) return refuse(ERR_BAD_INPUT);
            F.names.emplace_back((const char*)raw + at, (size_t)((const uint8_t*)z - (raw + at)));
            at = (size_t)((const uint8_t*)z - raw) + 1;
        }
        r.at = end;
    }
    F.nRef = nRef;
    std::vector<std::pair<int32_t, size_t>> order;                              // (bin, where its chunks start in the bytes)
    std::vector<int32_t> nChunk;
    for (int32_t t = 0; t < nRef; ++t) {
        const int32_t nBin = (int32_t)r.u32();
        if (!r.ok || nBin < 0) return refuse(ERR_BAD_INPUT);
        order.clear(); nChunk.clear();
        for (int32_t b = 0; b < nBin; ++b) {
            const uint32_t bin = r.u32();
            const int32_t n = (int32_t)r.u32();
            if (!r.ok || n < 0 || !r.need(16ull * (uint64_t)n)) return refuse(ERR_BAD_INPUT);
            if (bin > (uint32_t)MAX_BIN) return refuse(ERR_BAD_INPUT);
            if (bin != (uint32_t)MAX_BIN) { order.emplace_back((int32_t)bin, r.at); nChunk.push_back(n); }  // (the pseudo-bin is dropped here)
            r.at += 16 * (size_t)n;
        }
        std::vector<size_t> by(order.size());
        for (size_t k = 0; k < by.size(); ++k) by[k] = k;
        std::sort(by.begin(), by.end(), [&](size_t a, size_t b) { return order[a].first < order[b].first; });
        for (size_t k = 0; k < by.size(); ++k) {
            if (k && order[by[k]].first == order[by[k - 1]].first) return refuse(ERR_BAD_INPUT);
            F.binId.push_back(order[by[k]].first);
            Reader c{raw, len, order[by[k]].second};
            for (int32_t j = 0; j < nChunk[by[k]]; ++j) { F.chunkU.push_back((int64_t)c.u64()); F.chunkV.push_back((int64_t)c.u64()); }
            F.binChunkFirst.push_back((int64_t)F.chunkU.size());
        }
        F.refBinFirst.push_back((int64_t)F.binId.size());
        const int32_t nIntv = (int32_t)r.u32();
        if (!r.ok || nIntv < 0 || !r.need(8ull * (uint64_t)nIntv)) return refuse(ERR_BAD_INPUT);
        int64_t last = 0;
        for (int32_t i = 0; i < nIntv; ++i) {
            const int64_t x = (int64_t)r.u64();
            if (x != 0) last = x;
            F.linFill.push_back(last);
        }
        F.refLinFirst.push_back((int64_t)F.linFill.size());
    }
    if (kind == KIND_BAI && len - r.at >= 8) F.noCoor = (int64_t)r.u64();
    return 0;
}

// the reference's three loops as they stand (index.c.pysam.c:853-866) over a list sorted by (u, v)
inline std::vector<Chunk> resolve_serial(std::vector<Chunk> off)
{
    if (off.empty()) return off;
    size_t n = off.size(), l = 0;
    for (size_t i = 1; i < n; ++i) if (off[l].second < off[i].second) off[++l] = off[i];                    // completely contained chunks
    n = l + 1;
    for (size_t i = 1; i < n; ++i) if (off[i - 1].second >= off[i].first) off[i - 1].second = off[i].first;     // overlaps
    l = 0;
    for (size_t i = 1; i < n; ++i) {                                                                        // chunks that meet in one block
        if (off[l].second >> 16 == off[i].first >> 16) off[l].second = off[i].second;
        else off[++l] = off[i];
    }
    off.resize(l + 1);
    return off;
}

// the same as three data-parallel steps: an exclusive prefix maximum of v and a compaction (chunk i goes when v[i] <= the largest v in
// front of it); an element-wise cut v[i] = min(v[i], u[i + 1]); segment heads (a chunk opens an output chunk exactly when
// v[i - 1] >> 16 != u[i] >> 16; the output chunk's end is the v of the last member of its run)
inline std::vector<Chunk> resolve_parallel(const std::vector<Chunk>& off)
{
    const size_t n = off.size();
    std::vector<uint64_t> before(n, 0);
    for (size_t i = 1; i < n; ++i) before[i] = std::max(before[i - 1], off[i - 1].second);
    std::vector<Chunk> kept;
    for (size_t i = 0; i < n; ++i) if (i == 0 || off[i].second > before[i]) kept.push_back(off[i]);
    std::vector<Chunk> cut(kept);
    for (size_t i = 0; i + 1 < kept.size(); ++i) cut[i].second = std::min(kept[i].second, kept[i + 1].first);
    std::vector<uint8_t> head(cut.size(), 0);
    for (size_t i = 0; i < cut.size(); ++i) head[i] = i == 0 || cut[i - 1].second >> 16 != cut[i].first >> 16;
    std::vector<Chunk> out;
    for (size_t i = 0; i < cut.size(); ++i) {
        if (head[i]) out.push_back(cut[i]);
        else out.back().second = cut[i].second;
    }
    return out;
}

// ... and as ONE scan, which is what the kernels run.  With M[i] the largest v in front of i (the exclusive prefix maximum): the last
// chunk kept in front of i holds M[i], so i is kept when v[i] > M[i]; the chunk in front of a kept i is cut to min(M[i], u[i]), so i
// opens an output chunk when M[i] >> 16 < u[i] >> 16; and the output chunk in front of that head ends at M[i] (below u[i] then), the
// last one at the largest v of all.  No compaction is needed: heads are ranked among themselves.
inline std::vector<Chunk> resolve_fused(const std::vector<Chunk>& off)
{
    std::vector<Chunk> out;
    uint64_t M = 0;
    for (size_t i = 0; i < off.size(); ++i) {
        const bool head = i == 0 || (off[i].second > M && M >> 16 < off[i].first >> 16);
        if (head) {
            if (i) out.back().second = M;
            out.push_back(off[i]);
        }
        M = i == 0 ? off[i].second : std::max(M, off[i].second);
    }
    if (!out.empty()) out.back().second = M;
    return out;
}

// The chunks a query gathers, unsorted: every chunk of every listed bin the reference holds with v > min_off.  tid inside the index,
// 0 <= beg < end.  Six searches in the reference's ascending bin ids, then consecutive bins up to each level range's top.
inline void gather(const Flat& F, int32_t tid, int32_t beg, int32_t end, std::vector<Chunk>& off)
{
    off.clear();
    const int64_t l0 = F.refLinFirst[(size_t)tid], slot = lin_slot(beg, F.refLinFirst[(size_t)tid + 1] - l0);
    const uint64_t minOff = slot < 0 ? 0 : (uint64_t)F.linFill[(size_t)(l0 + slot)];
    const int64_t b0 = F.refBinFirst[(size_t)tid], b1 = F.refBinFirst[(size_t)tid + 1];
    for (int level = 0; level < LEVELS; ++level) {
        int32_t lo, hi;
        level_range(level, beg, end, &lo, &hi);
        for (int64_t b = lower_bound(F.binId.data(), b0, b1, lo); b < b1 && F.binId[(size_t)b] <= hi; ++b)
            for (int64_t c = F.binChunkFirst[(size_t)b]; c < F.binChunkFirst[(size_t)b + 1]; ++c)
                if ((uint64_t)F.chunkV[(size_t)c] > minOff) off.emplace_back((uint64_t)F.chunkU[(size_t)c], (uint64_t)F.chunkV[(size_t)c]);
    }
}

// The host twin of one query of plat_index_query_batch: the count (COUNT_NO_ITER where the reference returns no iterator), the chunks
// appended to u / v, the gathered count.  ERR_INVALID for a tid outside the index (nothing appended).
inline int query(const Flat& F, int32_t tid, int32_t beg, int32_t end, std::vector<int64_t>& u, std::vector<int64_t>& v, int32_t* count, int32_t* gathered)
{
    *count = 0; *gathered = 0;
    if (tid < 0 || tid >= F.nRef) return ERR_INVALID;
    if (beg < 0) beg = 0;
    if (end < beg) { *count = COUNT_NO_ITER; return 0; }
    if (beg >= end) return 0;
    std::vector<Chunk> off;
    gather(F, tid, beg, end, off);
    *gathered = (int32_t)std::min<size_t>(off.size(), (size_t)INT32_MAX);
    std::sort(off.begin(), off.end());
    const std::vector<Chunk> out = resolve_parallel(off);
    for (const Chunk& c : out) { u.push_back((int64_t)c.first); v.push_back((int64_t)c.second); }
    *count = (int32_t)out.size();
    return 0;
}

}  // namespace idxq
#endif
