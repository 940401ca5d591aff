// rg_regions.hpp -- plat_call_bam_regions_rg / plat_call_bgzf_regions_rg (include/platypus_caller_rg.h): the record front ends for merged
// files, on front_end.hpp's frame.  The records of every file's fetch go to the device as they are, plat_bam_route_batch (the second branch
// of loadBAMData, platypusutils.pyx:573-666, on the device) routes them to samples by their RG field, and the decode takes the routed
// offsets where the route left them (rgRegroup: a RecordList): from there on each call is its pre-split neighbour (decodeAndStage).  The host
// never reads an aux byte.
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
static int rgTableUpload(FrontCall& F, const plat_bam_read_groups* g, RgTable& t)
{
    plat_caller* c = F.c;
    const std::string& entry = F.entry;
    const int n_samples = F.n_samples;
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
    t.ids = F.dev.upload(ids, F.z->stream); t.off = F.dev.upload(off, F.z->stream); t.sample = F.dev.upload(sample, F.z->stream);
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

// the route of a list's records (cap: how many the list has room for -- the find's count is still on its way) enqueued, its counts and
// status on their way back
static void rgRouteLaunch(FrontCall& F, const RgTable& t, const RecordList& L, long long cap, RgRouted& r)
{
    Slot& z = *F.z;
    FetchedDeviceBuffers& dev = F.dev;
    r = RgRouted();
    r.nStreams = L.nStreams(); r.cap = cap;
    r.outBegin.assign((size_t)r.nStreams * (size_t)F.n_samples + 1, 0);
    r.o.rec_off = dev.alloc<int64_t>((size_t)cap); r.o.rec_limit = dev.alloc<int64_t>((size_t)cap);
    r.o.out_begin = dev.alloc<int32_t>(r.outBegin.size()); r.o.rec_sample = dev.alloc<int32_t>((size_t)cap);
    r.o.status = dev.alloc<int64_t>(4); r.o.why = dev.alloc<int32_t>(1);
    plat_bam_route_in q;
    memset(&q, 0, sizeof q);
    q.n_records = (int32_t)cap; q.n_streams = r.nStreams; q.n_groups = t.nGroups; q.n_samples = F.n_samples;
    q.blob = L.blob; q.blob_len = L.bytes; q.rec_off = L.off; q.rec_end = L.limit; q.stream_begin = L.dBegin;
    q.group_ids = t.ids; q.group_off = t.off; q.group_sample = t.sample;
    ck(plat_bam_route_batch(z.ctx, &q, &r.o, z.stream), "plat_bam_route_batch");
    dev.download(r.outBegin, r.o.out_begin, z.stream);
    dev.download(r.status, r.o.status, 4, z.stream);
    dev.download(&r.why, r.o.why, 1, z.stream);
}

// a route's status block, read back: 0, or the error with its message (L: the list it routed; stream s = file s % n_files of the
// s / n_files-th loaded region)
static int rgRouteFailure(FrontCall& F, const RgRouted& r, const char* what, const RecordList& L, int n_files)
{
    if (r.status[0] == 0) return PLAT_OK;
    if (r.status[0] != PLAT_ERR_BAD_INPUT) { F.c->lastError = F.entry + ": plat_bam_route_batch refuses its arguments"; return (int)r.status[0]; }
    const long long who = r.status[1];
    const int s = (int)(std::upper_bound(L.begin.begin(), L.begin.end(), (int32_t)who) - L.begin.begin()) - 1;
    static const char* const why[] = {"", "has no RG field", "has an RG field that is no string (type Z or H)", "has an RG value that is not in the table",
                                      "has aux data that does not parse (a field of unknown type)", "has aux data that does not parse (a B array with a negative count)",
                                      "has aux data that runs past the record", "runs past its rec_len or its blob before its aux data starts"};
    F.c->lastError = F.entry + ": " + what + " record " + std::to_string(who - L.begin[(size_t)s]) + " of " + F.where(F.loadedRegion(s / n_files), s % n_files, "file") +
                     " " + (r.why >= 1 && r.why <= 7 ? why[r.why] : "is refused by the route");
    return PLAT_ERR_BAD_INPUT;
}
// both routes' verdicts, the fetched records' first
static int rgRouteFailures(FrontCall& F, const RgRouted& rf, const RecordList& fetched, const RgRouted& rb, const RecordList& broken, int n_files)
{
    const int rc = rgRouteFailure(F, rf, "fetched", fetched, n_files);
    return rc != PLAT_OK ? rc : rgRouteFailure(F, rb, "broken-mate", broken, n_files);
}

// The routed records of the list L as the decode's streams (loaded region, sample): the route leaves (region, file, sample); with one file
// that is the same list, with more the pieces are copied into (region, sample, file) order on the device.
static RecordList rgRegroup(FrontCall& F, const RgRouted& r, const RecordList& L, int n_files)
{
    Slot& z = *F.z;
    FetchedDeviceBuffers& dev = F.dev;
    const int n_samples = F.n_samples, nRegions = r.nStreams / n_files;
    const long long n = r.outBegin.back();
    RecordList out;
    out.blob = L.blob; out.bytes = L.bytes;
    if (n_files == 1) { out.begin = r.outBegin; out.off = r.o.rec_off; out.limit = r.o.rec_limit; return out; }
    out.begin.assign(1, 0);
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
            out.begin.push_back((int32_t)at);
        }
    if (!pieces.empty()) ck(plat_copy_pieces(z.ctx, (int)pieces.size(), longest, dev.upload(pieces, z.stream), (uint8_t*)both, z.stream), "plat_copy_pieces");
    out.off = both; out.limit = both + n;
    return out;
}

// a file's table: its own fields and its rec_len (PLAT_ERR_INVALID, with a message for the latter)
static bool rgRecordsValid(FrontCall& F, const plat_bam_file_records& t) {
    const plat_bam_records& r = t.records;
    if (!recordsValid(r)) return false;
    if (r.n_records && !t.rec_len) { F.c->lastError = F.entry + ": records without rec_len (a record's aux data ends where its block_size says)"; return false; }
    for (int i = 0; i < r.n_records; ++i)
        if (t.rec_len[i] < 32) { F.c->lastError = F.entry + ": rec_len " + std::to_string(t.rec_len[i]) + " of record " + std::to_string(i) + " is below the 32 fixed bytes"; return false; }
    return true;
}

}  // namespace plathost

CALLER_EXPORT int plat_call_bam_regions_rg(plat_caller* c, const plat_bam_rg_region* regions, int n_regions, int n_files,
                                           const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                                           plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                           plat_fetched_region_info* info, plat_caller_stats* stats)
{
    FrontCall F(c, "plat_call_bam_regions_rg", n_regions, n_samples, sample_names, options, qc, out_text, out_len, info, stats);
    int rc = F.open(regions, n_files >= 1, {(const void*)plat_bam_route_batch, (const void*)plat_bam_decode_batch, (const void*)plat_read_buffers_batch},
                    "plat_bam_route_batch");
    if (rc != PLAT_OK) return rc;
    FetchedStage& S = F.S;
    std::vector<const plat_bam_file_records*> fetched, broken;             // per (loaded region, file)
    long long nReads = 0, nBroken = 0;
    for (int k = 0; k < n_regions; ++k) {                                 // (the bail-out on the region's record count over all files: it does not depend on the routing)
        const plat_bam_rg_region& r = regions[k];
        if (!r.files) return PLAT_ERR_INVALID;
        long long total = 0;
        for (int f = 0; f < n_files; ++f) {
            for (const plat_bam_file_records* t : {&r.files[f].fetched, &r.files[f].broken_mates}) if (!rgRecordsValid(F, *t)) return PLAT_ERR_INVALID;
            total += r.files[f].fetched.records.n_records;
        }
        S.loaded[(size_t)k] = !F.drops(total);
        if (!S.loaded[(size_t)k]) continue;
        for (int f = 0; f < n_files; ++f) {
            fetched.push_back(&r.files[f].fetched); broken.push_back(&r.files[f].broken_mates);
            for (const plat_bam_file_records* t : {&r.files[f].fetched, &r.files[f].broken_mates}) S.linkBytes += t->records.n_records ? t->records.data_len : 0;
            nReads += r.files[f].fetched.records.n_records; nBroken += r.files[f].broken_mates.records.n_records;
        }
    }
    if ((rc = F.tooMany(nReads, nBroken, (long long)(fetched.size() / (size_t)n_files) * n_samples, INT_MAX / 4)) != PLAT_OK) return rc;
    return F.guarded([&] {
        RgTable table;
        int rc = rgTableUpload(F, groups, table);
        if (rc != PLAT_OK) return rc;
        S.linkBytes += table.bytes;
        RgRouted rf, rb;
        const RecordList uf = uploadRecords(*F.z, F.dev, fetched), ub = uploadRecords(*F.z, F.dev, broken);
        rgRouteLaunch(F, table, uf, uf.n(), rf);
        rgRouteLaunch(F, table, ub, ub.n(), rb);
        ck(plat_stream_sync(F.z->ctx, F.z->stream), "plat_stream_sync");   // the one wait in front of the decode: the routes' counts
        if ((rc = rgRouteFailures(F, rf, uf, rb, ub, n_files)) != PLAT_OK) return rc;
        return decodeAndStage(F, rgRegroup(F, rf, uf, n_files), [&] { return rgRegroup(F, rb, ub, n_files); });
    });
}

CALLER_EXPORT int plat_call_bgzf_regions_rg(plat_caller* c, const plat_bgzf_rg_region* regions, int n_regions, int n_files,
                                            const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                                            plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                            plat_fetched_region_info* info, plat_caller_stats* stats)
{
    FrontCall F(c, "plat_call_bgzf_regions_rg", n_regions, n_samples, sample_names, options, qc, out_text, out_len, info, stats);
    int rc = F.open(regions, n_files >= 1, {(const void*)plat_bam_route_batch, (const void*)plat_bgzf_inflate_batch, (const void*)plat_bam_find_records,
                                            (const void*)plat_bam_decode_batch, (const void*)plat_read_buffers_batch}, "plat_bam_route_batch");
    if (rc != PLAT_OK) return rc;
    FetchedStage& S = F.S;
    return F.guarded([&] {
        BgzfFront W(F, n_files, "file");                                  // (its units are the files)
        int rc;
        for (int k = 0; k < n_regions; ++k) {
            const plat_bgzf_rg_region& r = regions[k];
            if (!r.files) return PLAT_ERR_INVALID;
            W.addRegion(r.tid, r.itr_beg, r.itr_end);
            for (int f = 0; f < n_files; ++f) {
                const plat_bgzf_file& fl = r.files[f];
                if (fl.n_chunks < 0 || (fl.n_chunks && !fl.chunks) || !rgRecordsValid(F, fl.broken_mates)) return PLAT_ERR_INVALID;
                if ((rc = W.addUnit(k, f, fl.n_chunks, fl.chunks)) != PLAT_OK) return rc;
            }
        }
        RgTable table;
        if ((rc = rgTableUpload(F, groups, table)) != PLAT_OK) return rc;
        // upload, inflate, then find and route (the fetched records where the find leaves them, the broken mates of the same regions): back to back
        W.batch.inflate();
        RgRouted rf, rb;
        RecordList kept, ub;
        rc = W.findLoaded(kept, [&](const std::vector<int>& use) {
            rgRouteLaunch(F, table, kept, W.batch.capRecords, rf);
            std::vector<const plat_bam_file_records*> broken;
            for (int k = 0; k < n_regions; ++k)
                for (int f = 0; f < n_files && use[(size_t)k]; ++f) broken.push_back(&regions[k].files[f].broken_mates);
            ub = uploadRecords(*F.z, F.dev, broken);
            rgRouteLaunch(F, table, ub, ub.n(), rb);
        });
        if (rc != PLAT_OK) return rc;
        if ((rc = rgRouteFailures(F, rf, kept, rb, ub, n_files)) != PLAT_OK) return rc;
        S.linkBytes += W.loadedBytes(S.loaded) + ub.bytes + table.bytes;
        if ((rc = F.tooMany(kept.n(), ub.n(), (long long)(rf.nStreams / n_files) * n_samples, INT_MAX / 4)) != PLAT_OK) return rc;
        return decodeAndStage(F, rgRegroup(F, rf, kept, n_files), [&] { return rgRegroup(F, rb, ub, n_files); });
    });
}
