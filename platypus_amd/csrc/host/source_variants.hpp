// source_variants.hpp -- candidates from source VCF lines in the native region loop (include/platypus_caller_source.h):
//
//   VariantCandidateReader.Variants       src/python/variantutils.py:56-163   (the line loop :72-159 is plat_source_variants_batch on the
//                                                                               device, or the host parser below; set() and sorted() of :161 here)
//   generateVariantsInRegion's share      src/cython/variantcaller.pyx:490-493,521   (rawBamVariants + vcfFileVariants + assemblerVariants)
//
// A chunk that holds a region with source lines uploads the lines with the chunk, has them parsed on the device (one call per chunk) and
// takes the host's stage B (Chunk::eligibleDeviceB says no).  The host parser -- the same rule, source_rule.hpp, over lines found with
// memchr -- runs where the device library lacks the entry point (the CPU suite's stand-in device predates it: referenced weakly, as
// plat_bam_decode_batch), where PLAT_CALLER_HOST_SOURCE=1 is set, and as the kernel's A/B in the tests (plat_caller_debug_source_*).
// PLAT_SOURCE_PARSER_ONLY: the parser and the ordering alone, for a stand-alone program (tests/source_parse_driver.cpp).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../../include/platypus_mi355x.h"
#include "variants.hpp"
#include "../source_rule.hpp"
#ifndef PLAT_SOURCE_PARSER_ONLY
#include "caller_common.hpp"
#include "chunk.hpp"
#include "../../../include/platypus_caller_source.h"

#pragma weak plat_source_variants_batch
#endif

namespace plathost {

// what plat_source_variants_batch hands back, on the host
struct SourceAlleles {
    std::vector<int32_t> regionBegin, pos, nRem, nAdd, hash, line, stats;
    std::vector<int64_t> remOff, addOff;
    int64_t status[4] = {0, -1, 0, 0};
    size_t size() const { return pos.size(); }
};

// The host parser: plat_source_variants_batch's outputs for the same inputs (cap: its cap_variants; < 0: no limit).
inline void parseSourceLinesHost(const uint8_t* text, int64_t textLen, const int64_t* textOff, const int64_t* nameHash, int nRegions, int maxSize, int longHaps,
                                 int64_t cap, SourceAlleles& out)
{
    out = SourceAlleles();
    for (int k = 0; k < nRegions; ++k)
        if (textOff[k] < 0 || textOff[k + 1] < textOff[k] || textOff[k + 1] > textLen) { out.status[0] = PLAT_ERR_INVALID; return; }
    out.regionBegin.assign((size_t)nRegions + 1, 0);
    out.stats.assign((size_t)nRegions * 4, 0);
    int64_t total = 0, lines = 0;
    uint64_t firstBad = ~0ull;
    for (int k = 0; k < nRegions; ++k) {
        out.regionBegin[(size_t)k] = (int32_t)((cap >= 0 && total > cap) ? cap : total);
        const int64_t end = textOff[k + 1];
        int32_t lineNo = 0;
        for (int64_t a = textOff[k]; a < end; ++lineNo) {
            const void* nl = memchr(text + a, '\n', (size_t)(end - a));
            const int64_t next = nl ? (const uint8_t*)nl - text + 1 : end;
            const srcrule::LineResult r = srcrule::parse_line(text, a, end, maxSize, longHaps, [&](int32_t p, int64_t ro, int32_t nr, int64_t ao, int32_t na) {
                if (cap < 0 || total < cap) {
                    out.pos.push_back(p); out.remOff.push_back(ro); out.nRem.push_back(nr); out.addOff.push_back(ao); out.nAdd.push_back(na);
                    out.hash.push_back(srcrule::py2_variant_hash32((uint64_t)nameHash[k], p, text + ro, nr, text + ao, na));
                    out.line.push_back(lineNo);
                }
                ++total;
            });
            int32_t* s = &out.stats[(size_t)k * 4];
            ++s[0];
            if (r.verdict == srcrule::LINE_SKIPPED) ++s[1];
            if (r.verdict == srcrule::LINE_INVALID) ++s[2];
            s[3] += r.oversize;
            if (r.verdict == srcrule::LINE_BAD) firstBad = std::min(firstBad, ((uint64_t)(uint32_t)k << 32) | (uint32_t)lineNo);
            a = next;
        }
        lines += out.stats[(size_t)k * 4];
    }
    out.regionBegin[(size_t)nRegions] = (int32_t)((cap >= 0 && total > cap) ? cap : total);
    out.status[0] = firstBad != ~0ull ? PLAT_ERR_BAD_INPUT : (cap >= 0 && total > cap) ? PLAT_ERR_OVERFLOW : 0;
    out.status[1] = firstBad != ~0ull ? (int64_t)firstBad : -1;
    out.status[2] = total; out.status[3] = lines;
}

// sorted(list(set(varList))) (variantutils.py:161) for the alleles [first, last) of one region, as indices: the Python-2 set replayed
// (setobject.c: alleles inserted in emission order, probed with the hash the parser computed -- Variant.__hash__, sign-extended; equal =
// position, removed and added all match; the first one is kept; iteration = slot order, as py2_dict_slot_order), then a stable sort by
// Variant.__richcmp__'s < (refPos, varType, nRemoved: variant.pyx:304-315).  Ties keep set order: that decides the order of two records
// at one position.
inline std::vector<int> sourceSetSorted(const uint8_t* text, const SourceAlleles& a, int first, int last) {
    auto hashOf = [&](int i) { return (uint64_t)(int64_t)a.hash[(size_t)i]; };
    auto same = [&](int x, int y) {
        return a.pos[(size_t)x] == a.pos[(size_t)y] && a.nRem[(size_t)x] == a.nRem[(size_t)y] && a.nAdd[(size_t)x] == a.nAdd[(size_t)y] &&
               memcmp(text + a.remOff[(size_t)x], text + a.remOff[(size_t)y], (size_t)a.nRem[(size_t)x]) == 0 &&
               memcmp(text + a.addOff[(size_t)x], text + a.addOff[(size_t)y], (size_t)a.nAdd[(size_t)x]) == 0;
    };
    std::vector<int> table(8, -1);
    auto slot = [&](const std::vector<int>& t, int key) {
        const uint64_t h = hashOf(key), mask = t.size() - 1;
        uint64_t i = h & mask, perturb = h;
        while (t[i & mask] >= 0 && !(hashOf(t[i & mask]) == h && same(t[i & mask], key))) { i = 5 * i + perturb + 1; perturb >>= 5; }
        return (size_t)(i & mask);
    };
    size_t used = 0;
    for (int key = first; key < last; ++key) {
        const size_t j = slot(table, key);
        if (table[j] >= 0) continue;
        table[j] = key;
        ++used;
        if (used * 3 >= table.size() * 2) {
            size_t size = 8;
            while (size <= used * (used > 50000 ? 2 : 4)) size <<= 1;
            std::vector<int> grown(size, -1);
            for (int k : table) if (k >= 0) grown[slot(grown, k)] = k;
            table.swap(grown);
        }
    }
    std::vector<int> order;
    order.reserve(used);
    for (int k : table) if (k >= 0) order.push_back(k);
    auto typeOf = [&](int i) {
        const int nr = a.nRem[(size_t)i], na = a.nAdd[(size_t)i];
        return nr == na ? (na == 1 ? SNP : MNP) : nr == 0 ? INS : na == 0 ? DEL : REP;
    };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        if (a.pos[(size_t)x] != a.pos[(size_t)y]) return a.pos[(size_t)x] < a.pos[(size_t)y];
        if (typeOf(x) != typeOf(y)) return typeOf(x) < typeOf(y);
        return a.nRem[(size_t)x] < a.nRem[(size_t)y];
    });
    return order;
}

}  // namespace plathost

#ifndef PLAT_SOURCE_PARSER_ONLY
namespace plathost {
// -- A4: the chunk's source lines -> RegionWork::srcVariants (FILE_VAR, no supporting reads), region by region
inline void Chunk::sourceCandidates() {
    size_t bytes = 0;
    for (const RegionWork* r : regions) bytes += (size_t)r->srcLen;
    if (!bytes) return;
    const auto t0 = Clock::now();
    Slot& z = s;
    const int n = (int)regions.size();
    std::vector<int64_t> off((size_t)n + 1, 0), nameHash((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        off[(size_t)k + 1] = off[(size_t)k] + regions[(size_t)k]->srcLen;
        nameHash[(size_t)k] = (int64_t)py2_string_hash(regions[(size_t)k]->in->chrom ? std::string(regions[(size_t)k]->in->chrom) : std::string());
    }
    const int64_t textLen = off[(size_t)n];
    SourceAlleles got;                                                  // the chunk's alleles; their offsets index the text of their own region
    const bool onDevice = plat_source_variants_batch && !o.sw.hostSource;
    auto refuse = [&](int64_t where) {                                  // a line pysam would raise on ends the call, named
        const RegionWork& r = *regions[(size_t)((uint64_t)where >> 32)];
        throw std::runtime_error(std::string("source lines of region ") + (r.in->chrom ? r.in->chrom : "?") + ":" + std::to_string(r.in->start) + "-" + std::to_string(r.in->end) +
                                 ", line " + std::to_string((uint32_t)where) + ": fewer than five columns or no usable POS");
    };
    if (!onDevice) {
        // region by region, where the caller's lines lie
        got.regionBegin.assign(1, 0);
        for (int k = 0; k < n; ++k) {
            const RegionWork& r = *regions[(size_t)k];
            SourceAlleles one;
            const int64_t own[2] = {0, r.srcLen};
            parseSourceLinesHost((const uint8_t*)r.srcText, r.srcLen, own, &nameHash[(size_t)k], 1, o.maxSize, o.srcLongHaps, -1, one);
            if (one.status[0] == PLAT_ERR_BAD_INPUT) refuse(((int64_t)k << 32) | (int64_t)(uint32_t)one.status[1]);
            got.pos.insert(got.pos.end(), one.pos.begin(), one.pos.end()); got.nRem.insert(got.nRem.end(), one.nRem.begin(), one.nRem.end());
            got.nAdd.insert(got.nAdd.end(), one.nAdd.begin(), one.nAdd.end()); got.hash.insert(got.hash.end(), one.hash.begin(), one.hash.end());
            got.remOff.insert(got.remOff.end(), one.remOff.begin(), one.remOff.end()); got.addOff.insert(got.addOff.end(), one.addOff.begin(), one.addOff.end());
            got.regionBegin.push_back((int32_t)got.size());
            got.status[3] += one.status[3];
        }
    } else {
        z.src_text.reserve(z.ctx, (size_t)textLen + 16, false, true, z.stream);
        for (int k = 0; k < n; ++k)                                     // the lines go up as they are, from the caller's memory: the one pass over them
            if (regions[(size_t)k]->srcLen)
                ck(plat_memcpy_h2d(z.ctx, z.src_text.d + off[(size_t)k], regions[(size_t)k]->srcText, (size_t)regions[(size_t)k]->srcLen, z.stream), "plat_memcpy_h2d");
        int64_t cap = std::max<int64_t>(16384, textLen / 64);
        for (int attempt = 0;; ++attempt) {
            Layout LI, LO;
            LI.put(z.src_off, off); LI.put(z.src_hash, nameHash);
            LI.commit(z, z.a_srcin);
            LI.upload(z, z.a_srcin);
            LO.add(z.src_status, 4); LO.add(z.src_begin, (size_t)n + 1); LO.add(z.src_stats, (size_t)n * 4);
            LO.add(z.src_pos, (size_t)cap); LO.add(z.src_nrem, (size_t)cap); LO.add(z.src_nadd, (size_t)cap); LO.add(z.src_hashes, (size_t)cap);
            LO.add(z.src_remoff, (size_t)cap); LO.add(z.src_addoff, (size_t)cap); LO.add(z.src_line, (size_t)cap);
            LO.commit(z, z.a_srcout);
            plat_source_variants_in qi;
            memset(&qi, 0, sizeof qi);
            qi.n_regions = n; qi.maxSize = o.maxSize; qi.longHaps = o.srcLongHaps;
            qi.text = z.src_text.d; qi.text_len = textLen; qi.text_off = z.src_off.d; qi.name_hash = z.src_hash.d;
            plat_source_variants_out qo;
            memset(&qo, 0, sizeof qo);
            qo.cap_variants = cap; qo.region_begin = z.src_begin.d; qo.pos = z.src_pos.d; qo.rem_off = z.src_remoff.d; qo.n_rem = z.src_nrem.d;
            qo.add_off = z.src_addoff.d; qo.n_add = z.src_nadd.d; qo.hash = z.src_hashes.d; qo.line = z.src_line.d; qo.region_stats = z.src_stats.d;
            qo.status = z.src_status.d;
            ck(plat_source_variants_batch(z.ctx, &qi, &qo, z.stream), "plat_source_variants_batch");
            LO.downloadFirst(z, z.a_srcout, 3);                         // status, region_begin, the regions' counters: they say how much more to fetch
            z.sync("source lines");
            if (z.src_status.h[0] == PLAT_ERR_OVERFLOW && attempt == 0) {   // (the call counted every allele: once more with room)
                cap = z.src_status.h[2];
                std::lock_guard<std::mutex> g(stMutex);
                ++st.n_source_retries;
                continue;
            }
            break;
        }
        for (int q = 0; q < 4; ++q) got.status[q] = z.src_status.h[q];
        // nothing is fetched for a chunk that is refused: a refused line wins over an overflow, so status[2] may exceed the capacity there
        if (got.status[0] == PLAT_ERR_BAD_INPUT) refuse(got.status[1]);
        if (got.status[0] != PLAT_OK) throw DeviceError((int)got.status[0], "plat_source_variants_batch");
        const size_t m = (size_t)std::min<int64_t>(got.status[2], cap);
        got.regionBegin.assign(z.src_begin.h, z.src_begin.h + n + 1);
        if (m) {
            // the used part of each array (each has `cap` entries: the used parts do not lie back to back)
            auto down = [&](auto& v) { ck(plat_memcpy_d2h(z.ctx, v.h, v.d, m * sizeof(*v.h), z.stream), "plat_memcpy_d2h"); };
            down(z.src_pos); down(z.src_nrem); down(z.src_nadd); down(z.src_hashes); down(z.src_remoff); down(z.src_addoff);
            z.sync("source alleles");
            auto take = [&](auto& into, const auto& v) { into.assign(v.h, v.h + m); };
            take(got.pos, z.src_pos); take(got.nRem, z.src_nrem); take(got.nAdd, z.src_nadd); take(got.hash, z.src_hashes);
            take(got.remOff, z.src_remoff); take(got.addOff, z.src_addoff);
            for (int k = 0; k < n; ++k)                                 // offsets into the chunk's text -> into the region's own lines, where the caller holds them
                for (int i = got.regionBegin[(size_t)k]; i < got.regionBegin[(size_t)k + 1]; ++i) { got.remOff[(size_t)i] -= off[(size_t)k]; got.addOff[(size_t)i] -= off[(size_t)k]; }
        }
    }
    int64_t nVar = 0;
    for (int k = 0; k < n; ++k) {
        RegionWork& r = *regions[(size_t)k];
        const uint8_t* text = (const uint8_t*)r.srcText;
        for (int i : sourceSetSorted(text, got, got.regionBegin[(size_t)k], got.regionBegin[(size_t)k + 1]))
            r.srcVariants.push_back(r.pool.make(got.pos[(size_t)i], (const char*)text + got.remOff[(size_t)i], (size_t)got.nRem[(size_t)i],
                                                (const char*)text + got.addOff[(size_t)i], (size_t)got.nAdd[(size_t)i], 0, FILE_VAR));
        nVar += (int64_t)r.srcVariants.size();
    }
    std::lock_guard<std::mutex> g(stMutex);
    st.n_source_lines += got.status[3]; st.n_source_variants += nVar; st.seconds_source += secs(t0, Clock::now());
    if (onDevice) ++st.n_source_chunks_device;
}

}  // namespace plathost

// ---- the C entry points (include/platypus_caller_source.h) -----------------------------------------------------------------------------
CALLER_EXPORT int plat_caller_set_source_lines(plat_caller* c, const plat_source_lines* per_region, int n_regions, int longHaps) {
    if (!c || n_regions < 0 || (n_regions > 0 && !per_region)) return PLAT_ERR_INVALID;
    for (int k = 0; k < n_regions; ++k) if (per_region[k].len < 0 || (per_region[k].len > 0 && !per_region[k].text)) return PLAT_ERR_INVALID;
    c->sourceLines.assign(per_region, per_region + n_regions);
    std::vector<char>().swap(c->sourceText);                               // (lines plat_caller_set_source_blocks fetched earlier are replaced too)
    c->sourceSet = n_regions > 0;                                          // (an empty list takes back lines set earlier: the next call is one without source lines)
    c->sourceLongHaps = longHaps;
    return PLAT_OK;
}

// For the tests: the host parser over one blob (the kernel's A/B), arrays as plat_source_variants_out lists them; returns status[0].
CALLER_EXPORT int plat_caller_debug_source_parse(const uint8_t* text, int64_t text_len, const int64_t* text_off, const int64_t* name_hash, int n_regions, int maxSize,
                                                 int longHaps, int64_t cap_variants, int32_t* region_begin, int32_t* pos, int64_t* rem_off, int32_t* n_rem,
                                                 int64_t* add_off, int32_t* n_add, int32_t* hash, int32_t* line, int32_t* region_stats, int64_t* status) {
    if (n_regions < 0 || text_len < 0 || !text_off || !status || cap_variants < 0) return PLAT_ERR_INVALID;
    plathost::SourceAlleles a;
    plathost::parseSourceLinesHost(text, text_len, text_off, name_hash, n_regions, maxSize, longHaps, cap_variants, a);
    for (int q = 0; q < 4; ++q) status[q] = a.status[q];
    if (a.status[0] == PLAT_ERR_INVALID) return PLAT_ERR_INVALID;
    for (size_t k = 0; k < a.regionBegin.size(); ++k) region_begin[k] = a.regionBegin[k];
    for (size_t k = 0; k < a.stats.size(); ++k) region_stats[k] = a.stats[k];
    for (size_t i = 0; i < a.size(); ++i) {
        pos[i] = a.pos[i]; rem_off[i] = a.remOff[i]; n_rem[i] = a.nRem[i]; add_off[i] = a.addOff[i]; n_add[i] = a.nAdd[i]; hash[i] = a.hash[i]; line[i] = a.line[i];
    }
    return (int)a.status[0];
}
// ... and the order of :161 for n alleles given as the parser leaves them: out[0 .. return value) = indices in the order sorted(list(set())) yields
CALLER_EXPORT int plat_caller_debug_source_order(const uint8_t* text, int n, const int32_t* pos, const int64_t* rem_off, const int32_t* n_rem, const int64_t* add_off,
                                                 const int32_t* n_add, const int32_t* hash, int* out) {
    plathost::SourceAlleles a;
    a.pos.assign(pos, pos + n); a.remOff.assign(rem_off, rem_off + n); a.nRem.assign(n_rem, n_rem + n); a.addOff.assign(add_off, add_off + n);
    a.nAdd.assign(n_add, n_add + n); a.hash.assign(hash, hash + n);
    const std::vector<int> order = plathost::sourceSetSorted(text, a, 0, n);
    for (size_t i = 0; i < order.size(); ++i) out[i] = order[i];
    return (int)order.size();
}
#endif  // PLAT_SOURCE_PARSER_ONLY
