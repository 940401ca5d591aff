// rg_regions.hpp -- plat_call_bam_regions_rg / plat_call_bgzf_regions_rg (include/platypus_caller_rg.h): the record front ends for merged
// files.  The records of every file's fetch go to the device as they are, plat_bam_route_batch (the second branch of loadBAMData,
// platypusutils.pyx:573-666, on the device) routes them to samples by their RG field, and the decode takes the routed offsets where the
// route left them: from there on each call is its pre-split neighbour (bamStage, fetchedFinish).  The host never reads an aux byte.
// Included at the end of region_caller.cpp, after bgzf_regions.hpp.
#pragma once
#include <map>

#include "../../../include/platypus_caller_rg.h"

// referenced weakly, as plat_bam_decode_batch: the CPU suite's stand-in device library predates it
#pragma weak plat_bam_route_batch

namespace plathost {

// the call's read-group table on the device (uploaded once per call)
struct RgTable {
    int nGroups = 0;
    const uint8_t* ids = nullptr;
    const int32_t* off = nullptr;
    const int32_t* sample = nullptr;
    long long bytes = 0;
};

// the table checked (PLAT_ERR_INVALID with a message) and uploaded
static int rgTableUpload(plat_caller* c, const std::string& entry, const plat_bam_read_groups* g, int n_samples, Slot& z, FetchedDeviceBuffers& dev, RgTable& t)
{
    if (!g || g->n_groups < 0 || (g->n_groups && (!g->id || !g->sample))) { c->lastError = entry + ": no read-group table"; return PLAT_ERR_INVALID; }
    if (g->n_groups > PLAT_ROUTE_MAX_GROUPS || n_samples > PLAT_ROUTE_MAX_SAMPLES) {
        c->lastError = entry + ": the device routes up to " + std::to_string(PLAT_ROUTE_MAX_GROUPS) + " read groups to up to " +
                       std::to_string(PLAT_ROUTE_MAX_SAMPLES) + " samples";
        return PLAT_ERR_UNSUPPORTED;
    }
    std::vector<uint8_t> ids;
    std::vector<int32_t> off(1, 0), sample;
    std::map<std::string, int> seen;
    for (int i = 0; i < g->n_groups; ++i) {
        if (!g->id[i] || !g->id[i][0]) { c->lastError = entry + ": read group " + std::to_string(i) + " has a NULL or empty ID"; return PLAT_ERR_INVALID; }
        if (g->sample[i] < 0 || g->sample[i] >= n_samples) {
            c->lastError = entry + ": read group " + std::to_string(i) + " (" + g->id[i] + ") names sample " + std::to_string(g->sample[i]) + " of " + std::to_string(n_samples);
            return PLAT_ERR_INVALID;
        }
        const auto at = seen.emplace(g->id[i], g->sample[i]);
        if (!at.second && at.first->second != g->sample[i]) {
            c->lastError = entry + ": read group ID " + g->id[i] + " is listed twice with different samples (resolve duplicates as the reference's dict would)";
            return PLAT_ERR_INVALID;
        }
        ids.insert(ids.end(), (const uint8_t*)g->id[i], (const uint8_t*)g->id[i] + strlen(g->id[i]));
        if (ids.size() > (size_t)INT_MAX) { c->lastError = entry + ": the read-group IDs are too long"; return PLAT_ERR_OVERFLOW; }
        off.push_back((int32_t)ids.size()); sample.push_back(g->sample[i]);
    }
    t.nGroups = g->n_groups; t.bytes = (long long)ids.size() + 8ll * g->n_groups;
    t.ids = dev.upload(ids, z.stream); t.off = dev.upload(off, z.stream); t.sample = dev.upload(sample, z.stream);
    return PLAT_OK;
}

// one route call: its streams are (loaded region, file), its output the offsets and limits the decode takes
struct RgRouted {
    plat_bam_route_out o;
    int nStreams = 0;
    long long cap = 0;                                                   // the record capacity handed to the route
    int64_t status[4] = {0, -1, 0, 0};
    int32_t why = 0;
    std::vector<int32_t> outBegin;                                       // [nStreams * n_samples + 1]
    RgRouted() { memset(&o, 0, sizeof o); }
};

// the route of `cap` records (dOff / dEnd / dStreamBegin on the device) enqueued, its counts and status on their way back
static void rgRouteLaunch(Slot& z, FetchedDeviceBuffers& dev, const RgTable& t, int n_samples, const uint8_t* dBlob, long long bytes, const int64_t* dOff,
                          const int64_t* dEnd, long long cap, const int32_t* dStreamBegin, int nStreams, RgRouted& r)
{
    r.nStreams = nStreams; r.cap = cap;
    r.outBegin.assign((size_t)nStreams * (size_t)n_samples + 1, 0);
    r.o.rec_off = dev.alloc<int64_t>((size_t)cap); r.o.rec_limit = dev.alloc<int64_t>((size_t)cap);
    r.o.out_begin = dev.alloc<int32_t>(r.outBegin.size()); r.o.rec_sample = dev.alloc<int32_t>((size_t)cap);
    r.o.status = dev.alloc<int64_t>(4); r.o.why = dev.alloc<int32_t>(1);
    plat_bam_route_in q;
    memset(&q, 0, sizeof q);
    q.n_records = (int32_t)cap; q.n_streams = nStreams; q.n_groups = t.nGroups; q.n_samples = n_samples;
    q.blob = dBlob; q.blob_len = bytes; q.rec_off = dOff; q.rec_end = dEnd; q.stream_begin = dStreamBegin;
    q.group_ids = t.ids; q.group_off = t.off; q.group_sample = t.sample;
    ck(plat_bam_route_batch(z.ctx, &q, &r.o, z.stream), "plat_bam_route_batch");
    ck(plat_memcpy_d2h(z.ctx, r.outBegin.data(), r.o.out_begin, r.outBegin.size() * sizeof(int32_t), z.stream), "plat_memcpy_d2h");
    ck(plat_memcpy_d2h(z.ctx, r.status, r.o.status, sizeof r.status, z.stream), "plat_memcpy_d2h");
    ck(plat_memcpy_d2h(z.ctx, &r.why, r.o.why, sizeof r.why, z.stream), "plat_memcpy_d2h");
}

// a route's status block, read back: 0, or the error with its message (streamBegin: the route's streams on the host; stream s = file
// s % n_files of the s / n_files-th loaded region)
static int rgRouteFailure(plat_caller* c, const std::string& entry, const RgRouted& r, const char* what, const std::vector<int32_t>& streamBegin,
                          const FetchedStage& S, const std::vector<FetchedRegionHead>& heads, int n_regions, int n_files)
{
    if (r.status[0] == 0) return PLAT_OK;
    if (r.status[0] != PLAT_ERR_BAD_INPUT) { c->lastError = entry + ": plat_bam_route_batch refuses its arguments"; return (int)r.status[0]; }
    const long long who = r.status[1];
    const int s = (int)(std::upper_bound(streamBegin.begin(), streamBegin.end(), (int32_t)who) - streamBegin.begin()) - 1;
    int k = 0, left = s / std::max(n_files, 1);
    for (; k < n_regions; ++k) if (S.loaded[(size_t)k] && left-- == 0) break;
    const FetchedRegionHead& h = heads[(size_t)k];
    static const char* const why[] = {"", "has no RG field", "has an RG field that is no string (type Z or H)", "has an RG value that is not in the table",
                                      "has aux data that does not parse (a field of unknown type)", "has aux data that does not parse (a B array with a negative count)",
                                      "has aux data that runs past the record", "runs past its rec_len or its blob before its aux data starts"};
    c->lastError = entry + ": " + what + " record " + std::to_string(who - streamBegin[(size_t)s]) + " of region " + std::to_string(k) + " (" + (h.chrom ? h.chrom : "?") +
                   ":" + std::to_string(h.start) + "-" + std::to_string(h.end) + "), file " + std::to_string(s % std::max(n_files, 1)) + " " +
                   (r.why >= 1 && r.why <= 7 ? why[r.why] : "is refused by the route");
    return PLAT_ERR_BAD_INPUT;
}

// The routed records as the decode's streams (loaded region, sample): the route leaves (region, file, sample); with one file that is the
// same list, with more the pieces are copied into (region, sample, file) order on the device.  d.tableBegin and the offsets to decode.
static void rgRegroup(Slot& z, FetchedDeviceBuffers& dev, const RgRouted& r, int n_files, int n_samples, BamDecoded& d, const int64_t** dOff, const int64_t** dLimit)
{
    const int nRegions = r.nStreams / std::max(n_files, 1);
    const long long n = r.outBegin.back();
    if (n_files == 1) { d.tableBegin = r.outBegin; *dOff = r.o.rec_off; *dLimit = r.o.rec_limit; return; }
    d.tableBegin.assign(1, 0);
    std::vector<plat_unpack_piece> pieces;
    int64_t* both = dev.alloc<int64_t>(2 * (size_t)n);                   // one blob for both lists: the offsets in front, the limits behind them
    long long at = 0, longest = 0;
    for (int k = 0; k < nRegions; ++k)
        for (int m = 0; m < n_samples; ++m) {
            for (int f = 0; f < n_files; ++f) {
                const size_t key = ((size_t)k * n_files + f) * n_samples + m;
                const long long b = r.outBegin[key], cnt = r.outBegin[key + 1] - b;
                if (!cnt) continue;
                pieces.push_back(plat_unpack_piece{(const uint8_t*)(r.o.rec_off + b), at * 8, cnt * 8});
                pieces.push_back(plat_unpack_piece{(const uint8_t*)(r.o.rec_limit + b), (n + at) * 8, cnt * 8});
                at += cnt; longest = std::max(longest, cnt * 8);
            }
            d.tableBegin.push_back((int32_t)at);
        }
    if (!pieces.empty()) ck(plat_copy_pieces(z.ctx, (int)pieces.size(), longest, dev.upload(pieces, z.stream), (uint8_t*)both, z.stream), "plat_copy_pieces");
    *dOff = both; *dLimit = both + n;
}

// the records of the call's files (per stream: loaded region, file) as one blob on the device with offsets, ends and the streams
struct RgRecords {
    const uint8_t* dBlob = nullptr;
    long long bytes = 0, n = 0;
    const int64_t* dOff = nullptr;
    const int64_t* dEnd = nullptr;
    const int32_t* dStreamBegin = nullptr;
    std::vector<int32_t> streamBegin;
};

static void rgUpload(Slot& z, FetchedDeviceBuffers& dev, const std::vector<const plat_bam_file_records*>& tables, RgRecords& u)
{
    void* st = z.stream;
    for (const plat_bam_file_records* t : tables) { u.bytes += t->records.n_records ? t->records.data_len : 0; u.n += t->records.n_records; }
    uint8_t* dBlob = dev.alloc<uint8_t>((size_t)u.bytes);
    std::vector<int64_t> recOff, recEnd;
    recOff.reserve((size_t)u.n); recEnd.reserve((size_t)u.n);
    u.streamBegin.assign(1, 0);
    long long base = 0;
    for (const plat_bam_file_records* t : tables) {
        const plat_bam_records& r = t->records;
        if (r.n_records) {
            ck(plat_memcpy_h2d(z.ctx, dBlob + base, r.data, (size_t)r.data_len, st), "plat_memcpy_h2d(records)");
            for (int i = 0; i < r.n_records; ++i) {                        // (a record outside its own blob stays outside: the device refuses it)
                const int64_t o = r.rec_off[i], e = o + t->rec_len[i];
                const bool in = o >= 0 && e <= r.data_len;
                recOff.push_back(in ? base + o : -1); recEnd.push_back(in ? base + e : -1);
            }
            base += r.data_len;
        }
        u.streamBegin.push_back((int32_t)recOff.size());
    }
    u.dBlob = dBlob; u.dOff = dev.upload(recOff, st); u.dEnd = dev.upload(recEnd, st); u.dStreamBegin = dev.upload(u.streamBegin, st);
}

static bool rgRecordsValid(plat_caller* c, const std::string& entry, const plat_bam_file_records& t, int* rc) {
    const plat_bam_records& r = t.records;
    if (r.n_records < 0 || (r.n_records && (!r.data || !r.rec_off || r.data_len < 0))) { *rc = PLAT_ERR_INVALID; return false; }
    if (r.n_records && !t.rec_len) { c->lastError = entry + ": records without rec_len (a record's aux data ends where its block_size says)"; *rc = PLAT_ERR_INVALID; return false; }
    for (int i = 0; i < r.n_records; ++i)
        if (t.rec_len[i] < 32) { c->lastError = entry + ": rec_len " + std::to_string(t.rec_len[i]) + " of record " + std::to_string(i) + " is below the 32 fixed bytes"; *rc = PLAT_ERR_INVALID; return false; }
    return true;
}

}  // namespace plathost

CALLER_EXPORT int plat_call_bam_regions_rg(plat_caller* c, const plat_bam_rg_region* regions, int n_regions, int n_files,
                                           const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                                           plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                           plat_fetched_region_info* info, plat_caller_stats* stats)
{
    SourceLinesGuard sourceGuard(c);
    int rc = checkCallArgs(c, options, out_text, out_len, n_regions, n_samples);
    if (rc != PLAT_OK) return rc;
    if (!qc || n_files < 1 || (n_regions > 0 && !regions)) return PLAT_ERR_INVALID;
    const std::string entry = "plat_call_bam_regions_rg";
    if (!plat_bam_route_batch || !plat_bam_decode_batch || !plat_read_buffers_batch) {
        c->lastError = entry + ": the device library has no plat_bam_route_batch";
        return PLAT_ERR_UNSUPPORTED;
    }
    const auto t0 = Clock::now();
    // loadBAMData's bail-out (:538-541) on the region's record count over all files: it does not depend on the routing
    const double mr = options->maxReads;
    const long long maxReads = mr >= (double)INT_MAX ? INT_MAX : (mr <= (double)INT_MIN ? INT_MIN : (long long)mr);     // (cdef int maxReads)
    FetchedStage S;
    S.loaded.assign((size_t)n_regions, 0);
    std::vector<FetchedRegionHead> heads;
    std::vector<const plat_bam_file_records*> fetched, broken;             // per (loaded region, file)
    long long nReads = 0, nBroken = 0;
    for (int k = 0; k < n_regions; ++k) {
        const plat_bam_rg_region& r = regions[k];
        if (!r.files) return PLAT_ERR_INVALID;
        heads.push_back(FetchedRegionHead{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, r.dev_contig_seq});
        long long total = 0;
        for (int f = 0; f < n_files; ++f) {
            for (const plat_bam_file_records* t : {&r.files[f].fetched, &r.files[f].broken_mates}) if (!rgRecordsValid(c, entry, *t, &rc)) return rc;
            total += r.files[f].fetched.records.n_records;
        }
        S.loaded[(size_t)k] = !(total > 0 && total >= maxReads);
        if (!S.loaded[(size_t)k]) continue;
        for (int f = 0; f < n_files; ++f) {
            fetched.push_back(&r.files[f].fetched); broken.push_back(&r.files[f].broken_mates);
            for (const plat_bam_file_records* t : {&r.files[f].fetched, &r.files[f].broken_mates}) S.linkBytes += t->records.n_records ? t->records.data_len : 0;
            nReads += r.files[f].fetched.records.n_records; nBroken += r.files[f].broken_mates.records.n_records;
        }
    }
    const int nLoaded = (int)fetched.size() / n_files;
    const long long nStreamsLL = (long long)nLoaded * n_samples;
    if (nStreamsLL > INT_MAX / 4 || nReads > INT_MAX - 2 * nStreamsLL - 1 || nBroken > INT_MAX - nStreamsLL - 1) {
        c->lastError = entry + ": more reads than one call takes (call the region list in parts)";
        return PLAT_ERR_OVERFLOW;
    }
    const int nStreams = (int)nStreamsLL;
    Slot& z = *c->slots[0];
    FetchedDeviceBuffers dev(z.ctx);
    try {
        RgTable table;
        rc = rgTableUpload(c, entry, groups, n_samples, z, dev, table);
        if (rc != PLAT_OK) return rc;
        S.linkBytes += table.bytes;
        RgRecords uf, ub;
        RgRouted rf, rb;
        rgUpload(z, dev, fetched, uf);
        rgUpload(z, dev, broken, ub);
        rgRouteLaunch(z, dev, table, n_samples, uf.dBlob, uf.bytes, uf.dOff, uf.dEnd, uf.n, uf.dStreamBegin, nLoaded * n_files, rf);
        rgRouteLaunch(z, dev, table, n_samples, ub.dBlob, ub.bytes, ub.dOff, ub.dEnd, ub.n, ub.dStreamBegin, nLoaded * n_files, rb);
        ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");         // the one wait in front of the decode: the routes' counts
        rc = rgRouteFailure(c, entry, rf, "fetched", uf.streamBegin, S, heads, n_regions, n_files);
        if (rc == PLAT_OK) rc = rgRouteFailure(c, entry, rb, "broken-mate", ub.streamBegin, S, heads, n_regions, n_files);
        if (rc != PLAT_OK) return rc;
        S.nStreams = nStreams; S.N = (int)nReads; S.packed = false;
        BamDecoded F, B;
        const int64_t* dOff = nullptr; const int64_t* dLimit = nullptr;
        rgRegroup(z, dev, rf, n_files, n_samples, F, &dOff, &dLimit);
        bamDecodeLaunch(z, dev, uf.dBlob, uf.bytes, dOff, dLimit, nReads, F);
        rgRegroup(z, dev, rb, n_files, n_samples, B, &dOff, &dLimit);
        bamDecodeLaunch(z, dev, ub.dBlob, ub.bytes, dOff, dLimit, nBroken, B);
        ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");
        rc = bamDecodeFailure(c, entry, F, B, S, heads, n_regions, n_samples);
        if (rc != PLAT_OK) return rc;
        bamStage(z, dev, S, F, B, nReads, nBroken, nStreams);
    } catch (const DeviceError& e) {
        c->lastError = e.what();
        return e.code;
    }
    return fetchedFinish(c, "plat_call_bam_regions_rg", dev, S, heads, n_samples, sample_names, options, qc, out_text, out_len, info, stats, t0);
}

CALLER_EXPORT int plat_call_bgzf_regions_rg(plat_caller* c, const plat_bgzf_rg_region* regions, int n_regions, int n_files,
                                            const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                                            plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                            plat_fetched_region_info* info, plat_caller_stats* stats)
{
    SourceLinesGuard sourceGuard(c);
    int rc = checkCallArgs(c, options, out_text, out_len, n_regions, n_samples);
    if (rc != PLAT_OK) return rc;
    if (!qc || n_files < 1 || (n_regions > 0 && !regions)) return PLAT_ERR_INVALID;
    const std::string entry = "plat_call_bgzf_regions_rg";
    if (!plat_bam_route_batch || !plat_bgzf_inflate_batch || !plat_bam_find_records || !plat_bam_decode_batch || !plat_read_buffers_batch) {
        c->lastError = entry + ": the device library has no plat_bam_route_batch";
        return PLAT_ERR_UNSUPPORTED;
    }
    const auto t0 = Clock::now();
    const double mr = options->maxReads;
    const long long maxReads = mr >= (double)INT_MAX ? INT_MAX : (mr <= (double)INT_MIN ? INT_MIN : (long long)mr);     // (cdef int maxReads)
    FetchedStage S;
    S.loaded.assign((size_t)n_regions, 0);
    std::vector<FetchedRegionHead> heads;
    BgzfFront W;                                                          // (its units are the files)
    W.entry = entry; W.nUnits = n_files;
    for (int k = 0; k < n_regions; ++k) {
        const plat_bgzf_rg_region& r = regions[k];
        if (!r.files) return PLAT_ERR_INVALID;
        heads.push_back(FetchedRegionHead{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, r.dev_contig_seq});
        W.addRegion(r.tid, r.itr_beg, r.itr_end);
        for (int f = 0; f < n_files; ++f) {
            const plat_bgzf_file& fl = r.files[f];
            if (fl.n_chunks < 0 || (fl.n_chunks && !fl.chunks)) return PLAT_ERR_INVALID;
            if (!rgRecordsValid(c, entry, fl.broken_mates, &rc)) return rc;
            rc = W.addUnit(c, heads.back(), k, f, fl.n_chunks, fl.chunks);
            if (rc != PLAT_OK) return rc;
        }
    }
    auto files = [](std::string m) {                                      // (the front's messages call a unit a sample)
        for (size_t at = m.find(", sample "); at != std::string::npos; at = m.find(", sample ", at)) m.replace(at, 9, ", file ");
        return m;
    };
    Slot& z = *c->slots[0];
    void* st = z.stream;
    FetchedDeviceBuffers dev(z.ctx);
    try {
        RgTable table;
        rc = rgTableUpload(c, entry, groups, n_samples, z, dev, table);
        if (rc != PLAT_OK) return rc;
        // upload, inflate, then find and route (the fetched records where the find leaves them, the broken mates of the same regions): back to back
        W.inflate(z, dev);
        RgRouted rf, rb;
        RgRecords ub;
        auto pass = [&](const std::vector<int>& use) {
            const int n = W.find(z, dev, use);
            rf = RgRouted(); rb = RgRouted(); ub = RgRecords();
            rgRouteLaunch(z, dev, table, n_samples, W.io.data, W.inflated, W.fo.rec_off, W.fo.rec_limit, W.capRecords, W.fo.stream_begin, n, rf);
            std::vector<const plat_bam_file_records*> broken;
            for (int k = 0; k < n_regions; ++k)
                for (int f = 0; f < n_files && use[(size_t)k]; ++f) broken.push_back(&regions[k].files[f].broken_mates);
            rgUpload(z, dev, broken, ub);
            rgRouteLaunch(z, dev, table, n_samples, ub.dBlob, ub.bytes, ub.dOff, ub.dEnd, ub.n, ub.dStreamBegin, n, rb);
        };
        std::vector<int> all((size_t)n_regions, 1);
        pass(all);
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");                // the one wait in front of the decode: status blocks, kept counts, the routes' counts
        rc = W.firstFailure(c, heads);
        if (rc != PLAT_OK) { c->lastError = files(c->lastError); return rc; }
        if (W.bailOut(maxReads, S.loaded)) {                               // the loaded regions alone: a second find, a second route
            pass(S.loaded);
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
            if (W.findStatus[0] != 0) { c->lastError = entry + ": the record walk fails on its second run"; return (int)W.findStatus[0]; }
        }
        rc = rgRouteFailure(c, entry, rf, "fetched", W.keptBegin, S, heads, n_regions, n_files);
        if (rc == PLAT_OK) rc = rgRouteFailure(c, entry, rb, "broken-mate", ub.streamBegin, S, heads, n_regions, n_files);
        if (rc != PLAT_OK) return rc;
        S.linkBytes += W.loadedBytes(S.loaded) + ub.bytes + table.bytes;
        const long long nStreamsLL = (long long)(rf.nStreams / n_files) * n_samples;
        const long long nReads = W.keptBegin.back(), nBroken = ub.n;
        if (nStreamsLL > INT_MAX / 4 || nReads > INT_MAX - 2 * nStreamsLL - 1 || nBroken > INT_MAX - nStreamsLL - 1) {
            c->lastError = entry + ": more reads than one call takes (call the region list in parts)";
            return PLAT_ERR_OVERFLOW;
        }
        const int nStreams = (int)nStreamsLL;
        S.nStreams = nStreams; S.N = (int)nReads; S.packed = false;
        BamDecoded F, B;
        const int64_t* dOff = nullptr; const int64_t* dLimit = nullptr;
        rgRegroup(z, dev, rf, n_files, n_samples, F, &dOff, &dLimit);
        bamDecodeLaunch(z, dev, W.io.data, W.inflated, dOff, dLimit, nReads, F);
        rgRegroup(z, dev, rb, n_files, n_samples, B, &dOff, &dLimit);
        bamDecodeLaunch(z, dev, ub.dBlob, ub.bytes, dOff, dLimit, nBroken, B);
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        rc = bamDecodeFailure(c, entry, F, B, S, heads, n_regions, n_samples);
        if (rc != PLAT_OK) return rc;
        bamStage(z, dev, S, F, B, nReads, nBroken, nStreams);
    } catch (const DeviceError& e) {
        c->lastError = e.what();
        return e.code;
    }
    return fetchedFinish(c, "plat_call_bgzf_regions_rg", dev, S, heads, n_samples, sample_names, options, qc, out_text, out_len, info, stats, t0);
}
