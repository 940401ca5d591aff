// tabix_index.hpp -- the tabix index of a bgzipped VCF (plat_tabix_index_batch, include/platypus_mi355x.h has the rule in words):
// ti_index_core with ti_conf_vcf (src/tabix/index.c.pysam.c:320-393) over ti_readline (:86-120), get_intv (:227-241), insert_offset2
// (:266-286), merge_chunks (:288-307), fill_missing (:309-318) and bgzf_tell.  Plain C++ without a library.  Three parts:
//   the rule of one record (parse_record, reg2bin, virtual_offset): compiled for the device (plat_tbxindex.hip) and for the host;
//   the serial builder (build_serial): the host twin of the device call -- the same intermediate: runs, names, windows, status;
//   the finishing stage (finish, compress): shared by both paths -- runs grouped by (tid, bin), merge_chunks, fill_missing, the
//   first-record quirk, the serialised index and its BGZF form.  It is O(runs + windows) and never reads the text.
// host/tbi_out.hpp runs the twin under PLAT_CALLER_HOST_TBI=1; tests/tabix_index_host_driver.cpp builds this file alone under the sanitizers.
#pragma once
#include <stdint.h>
#include "tabix_rule.hpp"

namespace tbxindex {

// the status block, in 64-bit words
enum { ST_VERDICT = 0, ST_LINE = 1, ST_KIND = 2, ST_RECORDS = 3, ST_RUNS = 4, ST_CONTIGS = 5, ST_WINDOWS = 6, ST_END = 7, ST_FIRST0 = 8, ST_FIRST_BEG = 9,
       ST_FIRST_END = 10, ST_LINES = 11, ST_NAME_BYTES = 12, ST_WORDS = 13 };
// why a file is refused; where two hold of one line the lower number is reported
enum { KIND_COLUMNS = 1, KIND_WIDE = 2, KIND_NEGATIVE_END = 3, KIND_ORDER = 4, KIND_NAME_AGAIN = 5 };
constexpr int ERR_INVALID = -1, ERR_UNSUPPORTED = -6, ERR_OVERFLOW = -8, ERR_BAD_INPUT = -9;      // (PLAT_ERR_* of the same names)
constexpr int LIDX_SHIFT = 14;
constexpr int MAX_REF = 65536;                            // contigs one file may hold (every contig's name is compared with every earlier one's)
constexpr int64_t MAX_ADDR = (int64_t)1 << 47;            // a block address: 48 bits of a virtual offset, kept positive in an int64

struct Record { int64_t nameLen; int32_t beg, end; int32_t kind; };      // kind: 0 or why the line is refused

// The record text[s, e) (e: its '\n' or the end of the data; its first byte is not '#').  Columns 1, 2, 4 and 8 are read and nothing
// behind the tab that ends column 8: ti_get_intv's VCF preset, as tbxrule::line_verdict restates it for the fetch.
TBX_FN Record parse_record(const uint8_t* text, int64_t s, int64_t e) {
    Record r = {0, 0, 0, 0};
    int id = 1;
    bool wide = false;
    int64_t b = 0, en = -1, colAt = s;
    for (int64_t i = s; i <= e && id <= 8; ++i) {
        if (i < e && text[i] != '\t' && text[i] != 0) continue;
        if (id == 1) r.nameLen = i - colAt;
        else if (id == 2) {
            const int64_t v = tbxrule::strtol0(text, colAt, e, &wide);         // (runs on to the line's end: a tab is white space)
            b = v - 1 < 0 ? 0 : v - 1;
            en = v < 1 ? 1 : v;
        } else if (id == 4) {
            if (colAt < i) en = b + (i - colAt);
        } else if (id == 8) {
            int64_t at = tbxrule::find_in(text, colAt, i, "END=", 4);
            if (at == colAt) at += 4;
            else if (at >= 0) { at = tbxrule::find_in(text, colAt, i, ";END=", 5); if (at >= 0) at += 5; }
            if (at >= 0) en = tbxrule::strtol0(text, at, i, &wide);
        }
        colAt = i + 1;
        ++id;
    }
    if (id <= 2) { r.kind = KIND_COLUMNS; return r; }
    if (wide || en > tbxrule::INT_LIMIT) { r.kind = KIND_WIDE; return r; }
    r.beg = (int32_t)b; r.end = (int32_t)en;
    if (en < 0) r.kind = KIND_NEGATIVE_END;
    return r;
}

// ti_reg2bin, in unsigned 32-bit arithmetic as the reference has it (end 0 wraps)
TBX_FN int32_t reg2bin(int32_t beg_, int32_t end_) {
    const uint32_t beg = (uint32_t)beg_, end = (uint32_t)end_ - 1u;
    if (beg >> 14 == end >> 14) return (int32_t)(4681u + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int32_t)(585u + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int32_t)(73u + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int32_t)(9u + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int32_t)(1u + (beg >> 26));
    return 0;
}
TBX_FN int32_t first_window(int32_t beg) { return beg >> LIDX_SHIFT; }
TBX_FN int32_t last_window(int32_t end) { return (int32_t)(((int64_t)end - 1) >> LIDX_SHIFT); }      // (signed: end 0 gives -1)

// the block of inflated offset t: the last b in [0, n_blocks) with out_off[b] <= t (out_off ascends from 0; n_blocks > 0)
TBX_FN int block_of(const int64_t* out_off, int n_blocks, int64_t t) {
    int lo = 0, hi = n_blocks;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (out_off[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}
TBX_FN int64_t virtual_offset(const int64_t* out_off, const int64_t* blk_addr, int n_blocks, int64_t t) {
    const int b = block_of(out_off, n_blocks, t);
    return (int64_t)(((uint64_t)blk_addr[b] << 16) | (uint64_t)(t - out_off[b]));
}
// what one entry of the geometry must satisfy: out_off from 0 in steps of at most 65536, block addresses ascending below 2^47
TBX_FN bool geometry_ok(const int64_t* out_off, const int64_t* blk_addr, int n_blocks, int64_t data_len, int b) {
    if (b == 0 && out_off[0] != 0) return false;
    if (blk_addr[b] < 0 || blk_addr[b] >= MAX_ADDR) return false;
    if (b == n_blocks) return out_off[b] <= data_len;
    const int64_t step = out_off[b + 1] - out_off[b];
    return step >= 0 && step <= 65536 && out_off[b] >= 0 && blk_addr[b + 1] >= blk_addr[b];
}

}  // namespace tbxindex

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace tbxindex {

// what the device call and the serial builder leave for the finishing stage
struct Intermediate {
    std::vector<int32_t> runTid, runBin;                  // the runs in file order
    std::vector<int64_t> runU;
    std::vector<int64_t> nameOff;                         // [contigs] into the data
    std::vector<int32_t> nameLen;
    std::vector<uint8_t> nameBytes;                       // the names back to back in tid order
    std::vector<int64_t> linFirst;                        // [contigs + 1] into lin
    std::vector<int64_t> lin;                             // the windows' first offsets, 0: unset
    int64_t status[ST_WORDS];
    void clear() { runTid.clear(); runBin.clear(); runU.clear(); nameOff.clear(); nameLen.clear(); nameBytes.clear(); linFirst.assign(1, 0); lin.clear(); memset(status, 0, sizeof status); status[ST_LINE] = -1; }
};

// The serial statement of the rule over data[0, out_off[n_blocks]).  A refused file leaves the verdict, the line and the kind in the
// status block and nothing else.
inline void build_serial(const uint8_t* data, int64_t data_len, const int64_t* out_off, const int64_t* blk_addr, int n_blocks, Intermediate& I) {
    I.clear();
    if (n_blocks < 0 || !blk_addr || (n_blocks > 0 && (!out_off || !data))) { I.status[ST_VERDICT] = ERR_INVALID; return; }
    for (int b = 0; b <= n_blocks && n_blocks > 0; ++b)
        if (!geometry_ok(out_off, blk_addr, n_blocks, data_len, b)) { I.status[ST_VERDICT] = ERR_INVALID; return; }
    if (n_blocks == 0 && (blk_addr[0] < 0 || blk_addr[0] >= MAX_ADDR)) { I.status[ST_VERDICT] = ERR_INVALID; return; }
    const int64_t total = n_blocks ? out_off[n_blocks] : 0;
    const int64_t endOff = (int64_t)((uint64_t)blk_addr[n_blocks] << 16);
    auto refuse = [&](int64_t line, int kind) { I.clear(); I.status[ST_VERDICT] = ERR_BAD_INPUT; I.status[ST_LINE] = line; I.status[ST_KIND] = kind; };
    std::map<std::string, int> seen;
    std::vector<std::vector<int64_t>> lin;
    std::vector<int32_t> nWin;
    int64_t lines = 0, records = 0, prevAt = -1, prevLen = 0;
    int32_t prevBeg = 0, prevBin = -1, tid = -1;
    for (int64_t p = 0; p < total;) {
        int64_t e = p;
        while (e < total && data[e] != '\n') ++e;
        ++lines;
        const int64_t s = p;
        p = e < total ? e + 1 : e;
        if (data[s] == '#') continue;
        const Record r = parse_record(data, s, e);
        if (r.kind) { refuse(lines, r.kind); return; }
        const bool change = prevAt < 0 || r.nameLen != prevLen || memcmp(data + s, data + prevAt, (size_t)prevLen) != 0;
        if (change) {
            const std::string name((const char*)data + s, (size_t)r.nameLen);
            if (seen.count(name)) { refuse(lines, KIND_NAME_AGAIN); return; }
            if ((int)seen.size() >= MAX_REF) { I.clear(); I.status[ST_VERDICT] = ERR_UNSUPPORTED; return; }
            seen[name] = ++tid;
            I.nameOff.push_back(s); I.nameLen.push_back((int32_t)r.nameLen);
            I.nameBytes.insert(I.nameBytes.end(), data + s, data + s + r.nameLen);
            lin.emplace_back(); nWin.push_back(0);
        } else if (prevBeg > r.beg) { refuse(lines, KIND_ORDER); return; }
        const int64_t u = virtual_offset(out_off, blk_addr, n_blocks, s);
        const int32_t bin = reg2bin(r.beg, r.end), w0 = first_window(r.beg), w1 = last_window(r.end);
        if (change || bin != prevBin) { I.runTid.push_back(tid); I.runBin.push_back(bin); I.runU.push_back(u); }
        std::vector<int64_t>& L = lin[(size_t)tid];
        if (w1 + 1 > (int32_t)L.size()) L.resize((size_t)w1 + 1, 0);
        for (int32_t w = w0; w <= w1; ++w) if (L[(size_t)w] == 0) L[(size_t)w] = u;
        if (w1 + 1 > nWin[(size_t)tid]) nWin[(size_t)tid] = w1 + 1;
        if (records == 0 && u == 0) { I.status[ST_FIRST0] = 1; I.status[ST_FIRST_BEG] = w0; I.status[ST_FIRST_END] = w1; }
        ++records;
        prevAt = s; prevLen = r.nameLen; prevBeg = r.beg; prevBin = bin;
    }
    for (size_t t = 0; t < lin.size(); ++t) {
        lin[t].resize((size_t)nWin[t], 0);
        I.lin.insert(I.lin.end(), lin[t].begin(), lin[t].end());
        I.linFirst.push_back((int64_t)I.lin.size());
    }
    I.status[ST_RECORDS] = records; I.status[ST_RUNS] = (int64_t)I.runU.size(); I.status[ST_CONTIGS] = (int64_t)I.nameOff.size();
    I.status[ST_WINDOWS] = (int64_t)I.lin.size(); I.status[ST_END] = endOff; I.status[ST_LINES] = lines; I.status[ST_NAME_BYTES] = (int64_t)I.nameBytes.size();
}

// the contigs' names of an intermediate
inline std::vector<std::string> names_of(const Intermediate& I) {
    std::vector<std::string> names;
    size_t at = 0;
    for (int32_t n : I.nameLen) { names.emplace_back((const char*)I.nameBytes.data() + at, (size_t)n); at += (size_t)n; }
    return names;
}

inline void put32(std::vector<uint8_t>& out, uint32_t v) { for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(v >> (8 * k))); }
inline void put64(std::vector<uint8_t>& out, uint64_t v) { for (int k = 0; k < 8; ++k) out.push_back((uint8_t)(v >> (8 * k))); }

// The finishing stage: the intermediate of an accepted file (status verdict 0) and its contigs' names to the index's bytes, before BGZF.
// Bins are written in ascending order (the reference writes its hash table's order; the format leaves it open).
inline std::vector<uint8_t> finish(const Intermediate& I, const std::vector<std::string>& names) {
    const size_t nRef = names.size(), nRuns = I.runU.size();
    std::vector<uint8_t> out;
    out.insert(out.end(), {'T', 'B', 'I', 1});
    put32(out, (uint32_t)nRef);
    for (uint32_t v : {2u, 1u, 2u, 0u, (uint32_t)'#', 0u}) put32(out, v);
    size_t lnm = 0;
    for (const std::string& n : names) lnm += n.size() + 1;
    put32(out, (uint32_t)lnm);
    for (const std::string& n : names) { out.insert(out.end(), n.begin(), n.end()); out.push_back(0); }
    // runs grouped by (tid, bin), file order kept inside a group
    std::vector<uint32_t> order(nRuns);
    for (size_t k = 0; k < nRuns; ++k) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return I.runTid[a] != I.runTid[b] ? I.runTid[a] < I.runTid[b] : (uint32_t)I.runBin[a] < (uint32_t)I.runBin[b];
    });
    size_t at = 0;
    for (size_t t = 0; t < nRef; ++t) {
        const size_t binCountAt = out.size();
        put32(out, 0);
        uint32_t nBin = 0;
        while (at < nRuns && I.runTid[order[at]] == (int32_t)t) {
            const int32_t bin = I.runBin[order[at]];
            std::vector<uint64_t> uv;                                         // merge_chunks: neighbours that meet in one block are joined
            for (; at < nRuns && I.runTid[order[at]] == (int32_t)t && I.runBin[order[at]] == bin; ++at) {
                const size_t k = order[at];
                const uint64_t u = (uint64_t)I.runU[k], v = (uint64_t)(k + 1 < nRuns ? I.runU[k + 1] : I.status[ST_END]);
                if (!uv.empty() && uv.back() >> 16 == u >> 16) uv.back() = v;
                else { uv.push_back(u); uv.push_back(v); }
            }
            put32(out, (uint32_t)bin); put32(out, (uint32_t)(uv.size() / 2));
            for (uint64_t x : uv) put64(out, x);
            ++nBin;
        }
        for (int k = 0; k < 4; ++k) out[binCountAt + k] = (uint8_t)(nBin >> (8 * k));
        const int64_t w0 = I.linFirst[t], n = I.linFirst[t + 1] - w0;
        std::vector<int64_t> L(I.lin.begin() + w0, I.lin.begin() + w0 + n);
        for (int64_t j = 1; j < n; ++j) if (L[(size_t)j] == 0) L[(size_t)j] = L[(size_t)j - 1];                       // fill_missing
        if (t == 0 && I.status[ST_FIRST0])                                    // the first record at offset 0: its windows are 0 whatever was filled in
            for (int64_t j = std::max<int64_t>(I.status[ST_FIRST_BEG], 0); j <= I.status[ST_FIRST_END] && j < n; ++j) L[(size_t)j] = 0;
        put32(out, (uint32_t)n);
        for (int64_t x : L) put64(out, (uint64_t)x);
    }
    return out;
}

}  // namespace tbxindex
#endif
