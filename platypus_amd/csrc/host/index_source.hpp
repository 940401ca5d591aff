// index_source.hpp -- plat_index_* and plat_caller_set_source_files (include/platypus_caller_index.h): a .tbi or .bai opened once --
// inflated (a .tbi: bgzf_blocks.hpp's host inflate over the file as one chunk) and flattened on the host by idxq::flatten (csrc/index_query.hpp), the tables uploaded --, a call's queries answered
// by plat_index_query_batch in one batch on slot 0's stream with one wait (queries the device hands over, and every query under
// PLAT_CALLER_HOST_INDEX=1, by idxq::query, the host twin), and source VCFs taken as files: per file one batch of queries, every chunk
// cut out of the file as tabixindex.cut_chunks cuts it (fetchIndexChunks: the one index fetch of a file, which the BAM files of
// bam_file.hpp and bam_mates.hpp go through too), and from there plat_caller_set_source_blocks.
// Included at the end of region_caller.cpp, after tabix_source.hpp.
#pragma once
#include "../../../include/platypus_caller_index.h"
#include "../index_query.hpp"

// referenced weakly, as plat_tabix_fetch_batch (tabix_source.hpp): the CPU suite's stand-in device library predates it
#pragma weak plat_index_query_batch

struct plat_index {
    plat_caller* c = nullptr;
    idxq::Flat F;
    std::unordered_map<std::string, int> tidOf;                           // (the first of equal names, as a list's index() finds it)
    plathost::FetchedDeviceBuffers tables;                                // the flat tables on the device, freed at close
    plat_index_query_in dev;                                              // ... as the device call takes them (the queries' fields unset)
    bool uploaded = false;
    std::vector<int64_t> first, u, v;                                     // the last query's answer
    std::vector<int32_t> count;
};

namespace plathost {

// a .tbi's bytes: every BGZF block inflated by the scalar driver; false when the bytes are no BGZF or a block does not inflate
inline bool inflateIndexBytes(const uint8_t* file, int64_t len, std::vector<uint8_t>& out)
{
    out.clear();
    if (len <= 0) return false;
    plat_bgzf_chunk ch;
    memset(&ch, 0, sizeof ch);
    ch.data = file; ch.data_len = len; ch.end_coffset = -1;
    std::string why;                                                      // (plat_index_open has one message for all of it)
    BgzfBlockList L("plat_index_open", [](const BgzfChunkAt&) { return std::string(); }, false, why);
    return L.add(0, 0, 0, ch) == PLAT_OK && L.inflated <= ((long long)1 << 31) && L.inflateOnHost(out) < 0;
}

inline void uploadIndexTables(plat_index& I)
{
    Slot& z = *I.c->slots[0];
    I.tables.ctx = z.ctx;
    void* st = z.stream;
    const idxq::Flat& F = I.F;
    memset(&I.dev, 0, sizeof I.dev);
    I.dev.n_ref = F.nRef; I.dev.n_bins = (int64_t)F.binId.size(); I.dev.n_chunks = (int64_t)F.chunkU.size(); I.dev.n_lin = (int64_t)F.linFill.size();
    I.dev.ref_bin_first = I.tables.upload(F.refBinFirst, st); I.dev.bin_id = I.tables.upload(F.binId, st);
    I.dev.bin_chunk_first = I.tables.upload(F.binChunkFirst, st); I.dev.chunk_u = I.tables.upload(F.chunkU, st); I.dev.chunk_v = I.tables.upload(F.chunkV, st);
    I.dev.ref_lin_first = I.tables.upload(F.refLinFirst, st); I.dev.lin_fill = I.tables.upload(F.linFill, st);
    ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
    I.uploaded = true;
}

// the host twin over queries [which]: their answers appended to u / v, their counts set
inline int twinQueries(plat_index& I, const std::vector<int>& which, const int32_t* tid, const int32_t* beg, const int32_t* end,
                       std::vector<std::vector<int64_t>>& us, std::vector<std::vector<int64_t>>& vs)
{
    for (size_t k = 0; k < which.size(); ++k) {
        const int q = which[k];
        int32_t gathered = 0;
        if (idxq::query(I.F, tid[q], beg[q], end[q], us[k], vs[k], &I.count[(size_t)q], &gathered) != 0) {
            I.c->lastError = "plat_index_query: query " + std::to_string(q) + " asks for tid " + std::to_string(tid[q]) + ", outside the index's " + std::to_string(I.F.nRef) + " references";
            return PLAT_ERR_INVALID;
        }
    }
    return PLAT_OK;
}

inline int queryIndex(plat_index& I, int n, const int32_t* tid, const int32_t* beg, const int32_t* end, plat_index_query_info* info)
{
    const auto t0 = Clock::now();
    plat_caller* c = I.c;
    if (info) memset(info, 0, sizeof *info);
    I.first.assign((size_t)n + 1, 0); I.u.clear(); I.v.clear(); I.count.assign((size_t)n, 0);
    const bool onHost = Switches::read().hostIndex;
    if (!onHost) { const int rc = needsEntryPoints(c, "plat_index_query", {(const void*)plat_index_query_batch}, "plat_index_query_batch"); if (rc != PLAT_OK) return rc; }
    std::vector<int> handed;
    int deviceCalls = 0;
    if (onHost) { for (int q = 0; q < n; ++q) handed.push_back(q); }
    else if (n > 0) {
        if (!I.uploaded) uploadIndexTables(I);
        Slot& z = *c->slots[0];
        FetchedDeviceBuffers dev(z);
        void* st = z.stream;
        plat_index_query_in in = I.dev;
        in.n_queries = n;
        const std::vector<int32_t> hTid(tid, tid + n), hBeg(beg, beg + n), hEnd(end, end + n);
        in.tid = dev.upload(hTid, st); in.beg = dev.upload(hBeg, st); in.end = dev.upload(hEnd, st);
        plat_index_query_out o;
        memset(&o, 0, sizeof o);
        o.count = dev.alloc<int32_t>((size_t)n); o.gathered = dev.alloc<int32_t>((size_t)n); o.q_first = dev.alloc<int64_t>((size_t)n + 1);
        o.status = dev.alloc<int64_t>(idxq::ST_WORDS);
        int64_t status[idxq::ST_WORDS] = {0};
        // a window of 100 kb comes back as a few chunks once neighbours are merged: room for sixteen a query at first, the count the device names after that
        int64_t cap = 16 * (int64_t)n + 1024;
        for (int attempt = 0;; ++attempt) {
            o.cap_chunks = cap;
            o.out_u = dev.alloc<int64_t>((size_t)cap); o.out_v = dev.alloc<int64_t>((size_t)cap);
            I.u.resize((size_t)cap); I.v.resize((size_t)cap);
            ck(plat_index_query_batch(z.ctx, &in, &o, st), "plat_index_query_batch");
            ++deviceCalls;
            dev.download(status, o.status, (size_t)idxq::ST_WORDS, st);
            dev.download(I.count, o.count, st); dev.download(I.first, o.q_first, st); dev.download(I.u, o.out_u, st); dev.download(I.v, o.out_v, st);
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");              // the one wait
            if (status[idxq::ST_VERDICT] != PLAT_ERR_OVERFLOW || attempt == 1) break;
            cap = status[idxq::ST_CHUNKS];
        }
        if (status[idxq::ST_VERDICT] == PLAT_ERR_INVALID && status[idxq::ST_QUERY] >= 0 && status[idxq::ST_QUERY] < n) {
            const int64_t q = status[idxq::ST_QUERY];
            c->lastError = "plat_index_query: query " + std::to_string(q) + " asks for tid " + std::to_string(tid[q]) + ", outside the index's " + std::to_string(I.F.nRef) + " references";
            return PLAT_ERR_INVALID;
        }
        if (status[idxq::ST_VERDICT] != 0) throw DeviceError((int)status[idxq::ST_VERDICT], "plat_index_query_batch");
        if (I.first[(size_t)n] != status[idxq::ST_CHUNKS] || I.first[(size_t)n] > cap) throw DeviceError(PLAT_ERR_INVALID, "plat_index_query_batch (counts that do not sum to the chunks)");
        I.u.resize((size_t)I.first[(size_t)n]); I.v.resize((size_t)I.first[(size_t)n]);
        for (int q = 0; q < n; ++q) if (I.count[(size_t)q] == idxq::COUNT_HANDED) handed.push_back(q);
    }
    if (!handed.empty()) {                                                 // the twin's answers spliced into the device's
        std::vector<std::vector<int64_t>> us(handed.size()), vs(handed.size());
        const int rc = twinQueries(I, handed, tid, beg, end, us, vs);
        if (rc != PLAT_OK) return rc;
        std::vector<int64_t> first((size_t)n + 1, 0), u, v;
        size_t k = 0;
        for (int q = 0; q < n; ++q) {
            if (k < handed.size() && handed[k] == q) { u.insert(u.end(), us[k].begin(), us[k].end()); v.insert(v.end(), vs[k].begin(), vs[k].end()); ++k; }
            else { u.insert(u.end(), I.u.begin() + I.first[(size_t)q], I.u.begin() + I.first[(size_t)q + 1]); v.insert(v.end(), I.v.begin() + I.first[(size_t)q], I.v.begin() + I.first[(size_t)q + 1]); }
            first[(size_t)q + 1] = (int64_t)u.size();
        }
        I.first.swap(first); I.u.swap(u); I.v.swap(v);
    }
    if (info) { info->queries = n; info->handed_over = (int64_t)handed.size(); info->chunks = I.first[(size_t)n]; info->device_calls = deviceCalls; info->seconds = secs(t0, Clock::now()); }
    return PLAT_OK;
}

// One chunk [u, v) of an index query cut out of the file's bytes as plat_bgzf_chunk takes it: from the block at u's coffset through the
// block at v's coffset, that block included when v's uoffset is non-zero, its length read from its own BSIZE.  false: the chunk does not
// begin and end at block headers inside the data.  (plat_caller_set_source_files for a .tbi, bam_file.hpp for a .bai.)
inline bool cutIndexChunk(const uint8_t* data, int64_t len, uint64_t u, uint64_t v, plat_bgzf_chunk& ch)
{
    const int64_t c0 = (int64_t)(u >> 16), c1 = (int64_t)(v >> 16);
    int64_t stop = c1;
    bgzf::BlockHead h;
    bool ok = c0 <= c1 && c1 <= len;
    if (ok && (v & 0xffff)) { ok = bgzf::parse_header(data, len, c1, &h) == 0; if (ok) stop = h.payload + h.payload_len + 8; }
    if (ok && stop > c0) ok = bgzf::parse_header(data, len, c0, &h) == 0;
    if (!ok) return false;
    memset(&ch, 0, sizeof ch);
    ch.data = data + c0; ch.data_len = stop - c0; ch.first_uoffset = (int32_t)(u & 0xffff); ch.end_coffset = c1 - c0; ch.end_uoffset = (int32_t)(v & 0xffff);
    return true;
}

// One file's share of a call's index fetch, for every entry point that takes whole files (plat_caller_set_source_files, bam_file.hpp,
// bam_mates.hpp): its queries answered in one batch (queryIndex), every chunk of every answer cut out of the file's bytes -- chunks[j]:
// query j's.  The messages carry the entry point's name; whereQuery(j) names query j's place in the call.
template <class Where>
inline int fetchIndexChunks(plat_caller* c, const std::string& entry, const uint8_t* data, int64_t len, plat_index& I, const std::vector<int32_t>& tid,
                            const std::vector<int32_t>& beg, const std::vector<int32_t>& end, Where&& whereQuery,
                            std::vector<std::vector<plat_bgzf_chunk>>& chunks, plat_index_query_info* info)
{
    const int rc = queryIndex(I, (int)tid.size(), tid.data(), beg.data(), end.data(), info);
    if (rc != PLAT_OK) { if (rc == PLAT_ERR_UNSUPPORTED) c->lastError = entry + ": the device library has no plat_index_query_batch"; return rc; }
    chunks.assign(tid.size(), {});
    for (size_t j = 0; j < tid.size(); ++j)
        for (int64_t at = I.first[j]; at < I.first[j + 1]; ++at) {
            const uint64_t u = (uint64_t)I.u[(size_t)at], v = (uint64_t)I.v[(size_t)at];
            plat_bgzf_chunk ch;
            if (!cutIndexChunk(data, len, u, v, ch)) {
                c->lastError = entry + ": chunk " + std::to_string(at - I.first[j]) + " of " + whereQuery(j) + " (virtual offsets " + std::to_string(u) + " .. " + std::to_string(v) +
                               ") does not begin and end at BGZF block headers inside the file's data";
                return PLAT_ERR_BAD_INPUT;
            }
            chunks[j].push_back(ch);
        }
    return PLAT_OK;
}

}  // namespace plathost

CALLER_EXPORT int plat_index_open(plat_caller* c, const uint8_t* bytes, size_t len, int kind, plat_index** out)
{
    if (!c || !out || (len > 0 && !bytes) || (kind != PLAT_INDEX_TBI && kind != PLAT_INDEX_BAI)) return PLAT_ERR_INVALID;
    *out = nullptr;
    return guardedEntry(c, "plat_index_open", [&] {
        std::unique_ptr<plat_index> I(new plat_index);
        I->c = c;
        std::vector<uint8_t> raw;
        if (kind == PLAT_INDEX_TBI && !inflateIndexBytes(bytes, (int64_t)len, raw)) {
            c->lastError = "plat_index_open: the .tbi's bytes are no BGZF stream that inflates (bad magic, no BC subfield, an invalid deflate stream or a CRC32 mismatch)";
            return (int)PLAT_ERR_BAD_INPUT;
        }
        const int rc = kind == PLAT_INDEX_TBI ? idxq::flatten(raw.data(), raw.size(), idxq::KIND_TBI, I->F) : idxq::flatten(bytes, len, idxq::KIND_BAI, I->F);
        if (rc == PLAT_ERR_UNSUPPORTED) { c->lastError = "plat_index_open: only the VCF preset of tabix and at most " + std::to_string(idxq::MAX_REF) + " references are handled"; return rc; }
        if (rc != 0) {
            c->lastError = "plat_index_open: the bytes are no index (a bad magic, bytes that end before a count says they should, a negative count, a bin twice in one reference or a bin id above 37450)";
            return rc;
        }
        for (size_t t = 0; t < I->F.names.size(); ++t) I->tidOf.emplace(I->F.names[t], (int)t);
        if (plat_index_query_batch) uploadIndexTables(*I);
        *out = I.release();
        return (int)PLAT_OK;
    });
}

CALLER_EXPORT int plat_index_close(plat_index* idx) { if (!idx) return PLAT_ERR_INVALID; delete idx; return PLAT_OK; }
CALLER_EXPORT int plat_index_n_refs(const plat_index* idx) { return idx ? idx->F.nRef : PLAT_ERR_INVALID; }
CALLER_EXPORT const char* plat_index_ref_name(const plat_index* idx, int tid) { return idx && tid >= 0 && (size_t)tid < idx->F.names.size() ? idx->F.names[(size_t)tid].c_str() : nullptr; }
CALLER_EXPORT int plat_index_tid(const plat_index* idx, const char* name)
{
    if (!idx || !name) return -1;
    const auto it = idx->tidOf.find(name);
    return it == idx->tidOf.end() ? -1 : it->second;
}

CALLER_EXPORT int plat_index_query(plat_index* idx, int n, const int32_t* tid, const int32_t* beg, const int32_t* end,
                                   const int64_t** first, const int64_t** u, const int64_t** v, const int32_t** count, plat_index_query_info* info)
{
    if (!idx || n < 0 || (n > 0 && (!tid || !beg || !end)) || !first || !u || !v || !count) return PLAT_ERR_INVALID;
    *first = nullptr; *u = nullptr; *v = nullptr; *count = nullptr;
    const int rc = guardedEntry(idx->c, "plat_index_query", [&] { return queryIndex(*idx, n, tid, beg, end, info); });
    if (rc != PLAT_OK) return rc;
    *first = idx->first.data(); *u = idx->u.data(); *v = idx->v.data(); *count = idx->count.data();
    return PLAT_OK;
}

CALLER_EXPORT int plat_caller_source_lines(const plat_caller* c, int region, const char** text, int64_t* len)
{
    if (!c || !text || !len || !c->sourceSet || region < 0 || (size_t)region >= c->sourceLines.size()) return PLAT_ERR_INVALID;
    *text = c->sourceLines[(size_t)region].text; *len = c->sourceLines[(size_t)region].len;
    return PLAT_OK;
}

CALLER_EXPORT int plat_caller_set_source_files(plat_caller* c, const plat_source_file* files, int n_files, const plat_source_region* regions, int n_regions,
                                               int longHaps, plat_source_blocks_info* info)
{
    if (!c || n_regions < 0 || n_files < 0 || (n_regions > 0 && !regions) || (n_files > 0 && !files)) return PLAT_ERR_INVALID;
    { SourceLinesGuard takeBack(c); }                                      // (whatever was set is gone, whichever way this call ends)
    if (info) memset(info, 0, sizeof *info);
    for (int f = 0; f < n_files; ++f) if (!files[f].index || files[f].index->c != c || files[f].data_len < 0 || (files[f].data_len && !files[f].data)) return PLAT_ERR_INVALID;
    for (int k = 0; k < n_regions; ++k) if (!regions[k].chrom) return PLAT_ERR_INVALID;
    if (n_regions == 0) return PLAT_OK;
    // per file: the regions it serves, their queries in one batch, every chunk cut out of the file
    struct Served { int region; std::vector<plat_bgzf_chunk> chunks; const char* name; };
    return guardedEntry(c, "plat_caller_set_source_files", [&] {
        std::vector<std::vector<Served>> served((size_t)n_files);
        for (int f = 0; f < n_files; ++f) {
            plat_index& I = *files[f].index;
            std::vector<int32_t> tid, beg, end;
            std::vector<Served>& S = served[(size_t)f];
            for (int k = 0; k < n_regions; ++k) {
                const int t = plat_index_tid(&I, regions[k].chrom);
                if (t < 0 || regions[k].end < std::max(regions[k].start, 0)) continue;            // (the reference's fetch raises: the file is skipped there)
                tid.push_back(t); beg.push_back(std::max(regions[k].start, 0)); end.push_back(regions[k].end);
                S.push_back(Served{k, {}, I.F.names[(size_t)t].c_str()});
            }
            std::vector<std::vector<plat_bgzf_chunk>> chunks;
            const int rc = fetchIndexChunks(c, "plat_caller_set_source_files", files[f].data, files[f].data_len, I, tid, beg, end,
                                            [&](size_t s) { return "region " + std::to_string(S[s].region) + ", file " + std::to_string(f); }, chunks, nullptr);
            if (rc != PLAT_OK) return rc;
            for (size_t s = 0; s < S.size(); ++s) S[s].chunks.swap(chunks[s]);
        }
        std::vector<std::vector<plat_tabix_fetch>> fetches((size_t)n_regions);
        std::vector<size_t> at((size_t)n_files, 0);
        for (int k = 0; k < n_regions; ++k)
            for (int f = 0; f < n_files; ++f) {
                std::vector<Served>& S = served[(size_t)f];
                if (at[(size_t)f] >= S.size() || S[at[(size_t)f]].region != k) continue;
                const Served& s = S[at[(size_t)f]++];
                plat_tabix_fetch ft;
                memset(&ft, 0, sizeof ft);
                ft.seq_name = s.name; ft.itr_beg = std::max(regions[k].start, 0); ft.itr_end = regions[k].end;
                ft.n_chunks = (int32_t)s.chunks.size(); ft.chunks = s.chunks.data();
                fetches[(size_t)k].push_back(ft);
            }
        std::vector<plat_source_blocks> per((size_t)n_regions);
        for (int k = 0; k < n_regions; ++k) per[(size_t)k] = plat_source_blocks{(int32_t)fetches[(size_t)k].size(), fetches[(size_t)k].data()};
        return plat_caller_set_source_blocks(c, per.data(), n_regions, longHaps, info);
    });
}
