// bam_mates.hpp -- plat_bam_files_mates_plan and plat_call_bam_files_mates (include/platypus_caller_bamfile.h): the broken-mate fetch of
// loadBAMData (platypusutils.pyx:522-559, :617-654) for whole files.  Two device batches on slot 0's stream, each the fetches of the whole
// call: bgzf_blocks.hpp's BgzfStreams (the chunks uploaded and inflated, plat_bam_find_records) with plat_bam_mates_batch behind it -- round
// one over the fetch plan's chunks for the mate coordinates, round two over the chunks of the merged queries for the mates themselves --
// and between them, on the host, csrc/mate_rule.hpp's sort and mergeQueries and one index fetch per file (fetchIndexChunks,
// index_source.hpp).  The call hands the plan's records to plat_call_bgzf_regions / _rg as broken_mates (callBamFilesWith, bam_file.hpp).
// Included at the end of region_caller.cpp, after bam_file.hpp.
#pragma once
#include "../mate_rule.hpp"

// referenced weakly, as plat_bam_find_records: the CPU suite's stand-in device library predates it
#pragma weak plat_bam_mates_batch

namespace plathost {

// One batch of fetches through the device.  A stream is one fetch: its window and its chunks, added in order; run() enqueues the shared
// batch and the mates pass behind it and waits once for the statuses and the streams' begins.
struct MatesBatch {
    plat_caller* c;
    const std::string entry;
    Slot& z;
    FetchedDeviceBuffers dev;
    const std::function<std::string(int)> whereStream;                    // "region K (chr:a-b), file F[, query Q (...)]"
    BgzfStreams batch;
    std::vector<BgzfStream> streams;
    RecordList kept;                                                      // the find's records, per stream
    plat_bam_mates_out mo;
    int64_t matesStatus[4] = {0, -1, 0, 0}, needBytes = 0;
    std::vector<int32_t> outBegin;                                        // per stream: the pass's outputs
    int deviceCalls = 0;

    MatesBatch(plat_caller* c_, const char* entry_, std::function<std::string(int)> where)
        : c(c_), entry(entry_), z(*c_->slots[0]), dev(z), whereStream(std::move(where)),
          batch(z, dev, entry, [this](const BgzfChunkAt& a) { return whereStream(a.region) + ", chunk " + std::to_string(a.chunk); }, c_->lastError)
    {
        memset(&mo, 0, sizeof mo);
    }

    int addStream(int32_t tid, int32_t beg, int32_t end, int n_chunks, const plat_bgzf_chunk* chunks)
    {
        const int s = (int)streams.size(), first = (int)batch.L.chunkAt.size();
        for (int q = 0; q < n_chunks; ++q) { const int rc = batch.L.add(s, 0, q, chunks[q]); if (rc != PLAT_OK) return rc; }
        streams.push_back(BgzfStream{first, (int)batch.L.chunkAt.size(), tid, beg, end});
        return PLAT_OK;
    }

    // upload, inflate, find, the pass; then the one wait and whatever a stage refused
    int run(int mode, const std::vector<int32_t>& want, const std::vector<int32_t>& lo, const std::vector<int32_t>& hi)
    {
        void* st = z.stream;
        const size_t n = streams.size();
        if (batch.recordCap() > INT_MAX) { c->lastError = entry + ": more records than one call takes (call the region list in parts)"; return PLAT_ERR_OVERFLOW; }
        batch.inflate();
        batch.find(streams, kept);
        const size_t capRecords = (size_t)batch.capRecords;
        plat_bam_mates_in mi;
        memset(&mi, 0, sizeof mi);
        mi.n_streams = (int)n; mi.n_records = (int32_t)capRecords; mi.mode = mode; mi.data = kept.blob; mi.data_len = kept.bytes;
        mi.rec_off = kept.off; mi.rec_limit = kept.limit; mi.stream_begin = kept.dBegin;
        mo.cap_records = batch.capRecords; mo.status = dev.alloc<int64_t>(4); mo.need_bytes = dev.alloc<int64_t>(1);
        int32_t* dBegin = dev.alloc<int32_t>(n + 1);
        if (mode == PLAT_MATES_COORDS) { mo.coords = dev.alloc<int32_t>(2 * capRecords); mo.coord_begin = dBegin; }
        else {
            mi.want_tid = dev.upload(want, st); mi.lo = dev.upload(lo, st); mi.hi = dev.upload(hi, st);
            mo.cap_bytes = kept.bytes; mo.out_data = dev.alloc<uint8_t>((size_t)kept.bytes + PLAT_BLOB_PAD);
            mo.out_rec_off = dev.alloc<int64_t>(capRecords); mo.out_rec_len = dev.alloc<int32_t>(capRecords); mo.out_mpos = dev.alloc<int32_t>(capRecords);
            mo.out_begin = dBegin;
        }
        ck(plat_bam_mates_batch(z.ctx, &mi, &mo, st), "plat_bam_mates_batch");
        deviceCalls += 3;
        outBegin.assign(n + 1, 0);
        dev.download(matesStatus, mo.status, 4, st); dev.download(&needBytes, mo.need_bytes, 1, st); dev.download(outBegin, dBegin, st);
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        const int rc = batch.firstFailure(whereStream);
        if (rc != PLAT_OK) return rc;
        // (the capacities are the find's and the inflated bytes: the pass has nothing left to refuse)
        if (matesStatus[0] != 0 || outBegin[n] != matesStatus[2]) throw DeviceError(matesStatus[0] != 0 ? (int)matesStatus[0] : PLAT_ERR_INVALID, "plat_bam_mates_batch");
        return PLAT_OK;
    }
};

}  // namespace plathost

struct plat_bam_mates_plan_impl : plat_bam_mates_plan {
    std::vector<plat_bam_mates> M;
    std::vector<std::vector<plat_bam_mate_query>> queries;                // per unit
    std::vector<std::vector<int64_t>> recOff;
    std::vector<std::vector<int32_t>> recLen;
    std::vector<int32_t> loadedRegions;
    std::vector<uint8_t> blob;                                            // the kept records of the call, stream after stream
    std::vector<std::vector<plat_bgzf_chunk>> chunks;                     // per second-round stream
};

namespace plathost {

inline int makeBamMatesPlan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions, const plat_bam_fetch_plan& X,
                            const plat_caller_options& options, plat_bam_mates_plan_impl& I)
{
    static const char* const entry = "plat_bam_files_mates_plan";
    const auto t0 = Clock::now();
    plat_caller* c = files[0]->c;
    plat_bam_mates_plan& p = I;
    memset(&p, 0, sizeof p);
    const size_t nUnits = (size_t)n_regions * (size_t)n_files;
    I.M.assign(nUnits, plat_bam_mates());
    for (plat_bam_mates& m : I.M) memset(&m, 0, sizeof m);
    I.queries.assign(nUnits, {}); I.recOff.assign(nUnits, {}); I.recLen.assign(nUnits, {});
    I.loadedRegions.assign((size_t)n_regions, 1);
    auto publish = [&] {
        for (size_t u = 0; u < nUnits; ++u) {
            plat_bam_mates& m = I.M[u];
            m.n_queries = (int32_t)I.queries[u].size(); m.queries = I.queries[u].data();
            m.mates.records.n_records = (int32_t)I.recOff[u].size(); m.mates.records.rec_off = I.recOff[u].data(); m.mates.rec_len = I.recLen[u].data();
        }
        p.n_regions = n_regions; p.n_files = n_files; p.units = I.M.data(); p.loaded = I.loadedRegions.data();
        p.seconds = secs(t0, Clock::now());
        return (int)PLAT_OK;
    };
    if (X.n_regions != n_regions || X.n_files != n_files || (nUnits && !X.fetches)) return PLAT_ERR_INVALID;
    int rc = needsEntryPoints(c, entry, {(const void*)plat_bam_mates_batch}, "plat_bam_mates_batch");
    if (rc == PLAT_OK) rc = needsEntryPoints(c, entry, {(const void*)plat_bgzf_inflate_batch}, "plat_bgzf_inflate_batch");
    if (rc == PLAT_OK) rc = needsEntryPoints(c, entry, {(const void*)plat_bam_find_records}, "plat_bam_find_records");
    if (rc != PLAT_OK) return rc;
    if (nUnits == 0) return publish();
    auto whereUnit = [&](int k, int f) {
        return "region " + std::to_string(k) + " (" + regions[k].chrom + ":" + std::to_string(regions[k].start) + "-" + std::to_string(regions[k].end) + "), file " + std::to_string(f);
    };

    // ---- round one: every fetch of the call, the mate coordinates of its kept records
    std::vector<mate::Coord> coords;
    std::vector<int32_t> coordBegin;
    {
        MatesBatch B(c, entry, [&](int s) { return whereUnit(s / n_files, s % n_files); });
        for (int k = 0; k < n_regions; ++k)
            for (int f = 0; f < n_files; ++f) {
                const plat_bam_fetch& ft = X.fetches[(size_t)k * n_files + f];
                if (ft.n_chunks < 0 || (ft.n_chunks && !ft.chunks)) return PLAT_ERR_INVALID;
                if ((rc = B.addStream(ft.tid, ft.itr_beg, ft.itr_end, ft.n_chunks, ft.chunks)) != PLAT_OK) return rc;
            }
        if ((rc = B.run(PLAT_MATES_COORDS, {}, {}, {})) != PLAT_OK) return rc;
        p.device_calls += B.deviceCalls;
        // loadBAMData's bail-out (:538-541) on the kept records of a region, summed over its files: no mate is fetched for it
        const long long maxReads = maxReadsOf(options);
        for (int k = 0; k < n_regions; ++k)
            I.loadedRegions[(size_t)k] = !dropsRegion((long long)B.kept.begin[(size_t)(k + 1) * n_files] - B.kept.begin[(size_t)k * n_files], maxReads);
        coordBegin = B.outBegin;
        std::vector<int32_t> flat(2 * (size_t)coordBegin.back());
        B.dev.download(flat, B.mo.coords, B.z.stream);
        if (!flat.empty()) ck(plat_stream_sync(B.z.ctx, B.z.stream), "plat_stream_sync");
        coords.resize(flat.size() / 2);
        for (size_t i = 0; i < coords.size(); ++i) coords[i] = mate::Coord{flat[2 * i], flat[2 * i + 1]};
    }

    // ---- the queries of every file and region: sorted by (name, mtid, mpos), merged
    struct Stream { int k, f, q; };
    std::vector<Stream> streams;
    for (int f = 0; f < n_files; ++f) {
        const plat_bamfile& B = *files[f];
        const int nRef = (int)B.refName.size();
        std::vector<int> order((size_t)nRef), rank((size_t)nRef, 0);      // a contig's place among the names, equal names sharing one
        for (int t = 0; t < nRef; ++t) order[(size_t)t] = t;
        std::sort(order.begin(), order.end(), [&](int a, int b) { const int cmp = B.refName[(size_t)a].compare(B.refName[(size_t)b]); return cmp != 0 ? cmp < 0 : a < b; });
        for (int i = 0, r = 0; i < nRef; ++i) {
            if (i && B.refName[(size_t)order[(size_t)i]] != B.refName[(size_t)order[(size_t)i - 1]]) ++r;
            rank[(size_t)order[(size_t)i]] = r;
        }
        for (int k = 0; k < n_regions; ++k) {
            const size_t u = (size_t)k * n_files + f;
            if (!I.loadedRegions[(size_t)k]) continue;
            mate::Coord* first = coords.data() + coordBegin[u];
            const long long n = (long long)coordBegin[u + 1] - coordBegin[u];
            for (long long j = 0; j < n; ++j) {
                const mate::Coord& m = first[j];
                if (m.mtid < 0 || m.mtid >= nRef) {
                    c->lastError = std::string(entry) + ": " + whereUnit(k, f) + ": coordinate " + std::to_string(j) + " names mate contig " + std::to_string(m.mtid) + ", outside the header's " +
                                   std::to_string(nRef) + " references";
                    return PLAT_ERR_BAD_INPUT;
                }
                if (m.mpos < 0) {
                    c->lastError = std::string(entry) + ": " + whereUnit(k, f) + ": record " + std::to_string(j) + " of those that give a mate coordinate has mate position " + std::to_string(m.mpos) +
                                   " on contig " + std::to_string(m.mtid) + ": no region string is defined for a negative position";
                    return PLAT_ERR_BAD_INPUT;
                }
            }
            I.M[u].n_coords = (int32_t)n;
            p.coords += n;
            std::stable_sort(first, first + n, [&](const mate::Coord& a, const mate::Coord& b) {
                return mate::coord_less(a, b, [&](int32_t x, int32_t y) { return rank[(size_t)x] - rank[(size_t)y]; });
            });
            mate::merge_queries(first, n, [&](int32_t x, int32_t y) { return rank[(size_t)x] == rank[(size_t)y]; }, [&](const mate::Query& q) {
                plat_bam_mate_query out;
                memset(&out, 0, sizeof out);
                out.tid = B.tidOf.find(B.refName[(size_t)q.mtid])->second; out.start = q.start; out.end = q.end;
                streams.push_back(Stream{k, f, (int)I.queries[u].size()});
                I.queries[u].push_back(out);
            });
            p.queries += (int64_t)I.queries[u].size();
        }
    }
    std::sort(streams.begin(), streams.end(), [](const Stream& a, const Stream& b) { return a.k != b.k ? a.k < b.k : a.f != b.f ? a.f < b.f : a.q < b.q; });
    if (streams.empty()) return publish();

    // ---- round two: per file one batch of index queries, every chunk cut; then one device batch for the mates
    auto whereStream = [&](int s) {
        const Stream& t = streams[(size_t)s];
        const plat_bam_mate_query& q = I.queries[(size_t)t.k * n_files + t.f][(size_t)t.q];
        return whereUnit(t.k, t.f) + ", query " + std::to_string(t.q) + " (" + files[t.f]->refName[(size_t)q.tid] + ":" + std::to_string(q.start) + "-" + std::to_string(q.end) + ")";
    };
    I.chunks.assign(streams.size(), {});
    std::vector<int32_t> wTid(streams.size()), wBeg(streams.size()), wEnd(streams.size());
    for (size_t s = 0; s < streams.size(); ++s) {
        const plat_bam_mate_query& q = I.queries[(size_t)streams[s].k * n_files + streams[s].f][(size_t)streams[s].q];
        wTid[s] = q.tid;
        mate::query_window(mate::Query{q.tid, q.start, q.end}, &wBeg[s], &wEnd[s]);
    }
    for (int f = 0; f < n_files; ++f) {
        std::vector<int32_t> tid, beg, end;
        std::vector<size_t> served;
        for (size_t s = 0; s < streams.size(); ++s)
            if (streams[s].f == f) { tid.push_back(wTid[s]); beg.push_back(wBeg[s]); end.push_back(wEnd[s]); served.push_back(s); }
        if (served.empty()) continue;
        plat_index_query_info qi;
        std::vector<std::vector<plat_bgzf_chunk>> chunks;
        rc = fetchIndexChunks(c, entry, files[f]->data, files[f]->len, *files[f]->index, tid, beg, end, [&](size_t j) { return whereStream((int)served[j]); }, chunks, &qi);
        if (rc != PLAT_OK) return rc;
        p.device_calls += qi.device_calls;
        for (size_t j = 0; j < served.size(); ++j) {
            for (const plat_bgzf_chunk& ch : chunks[j]) p.input_bytes += ch.data_len;
            I.chunks[served[j]].swap(chunks[j]);
        }
    }
    MatesBatch B(c, entry, whereStream);
    std::vector<int32_t> want, lo, hi;
    for (size_t s = 0; s < streams.size(); ++s) {
        const Stream& t = streams[s];
        if ((rc = B.addStream(wTid[s], wBeg[s], wEnd[s], (int)I.chunks[s].size(), I.chunks[s].data())) != PLAT_OK) return rc;
        want.push_back(X.fetches[(size_t)t.k * n_files + t.f].tid); lo.push_back(regions[t.k].start); hi.push_back(regions[t.k].end);
        p.chunks += (int64_t)I.chunks[s].size();
    }
    if ((rc = B.run(PLAT_MATES_FETCH, want, lo, hi)) != PLAT_OK) return rc;
    p.device_calls += B.deviceCalls;
    p.records_looked_at = B.matesStatus[3]; p.records_kept = B.matesStatus[2];
    // the one read-back of the kept records
    const size_t nKept = (size_t)B.outBegin.back();
    std::vector<int64_t> off(nKept);
    std::vector<int32_t> len(nKept), mpos(nKept);
    I.blob.assign((size_t)B.needBytes + PLAT_BLOB_PAD, 0);
    if (nKept) {
        B.dev.download(I.blob.data(), B.mo.out_data, (size_t)B.needBytes, B.z.stream);
        B.dev.download(off, B.mo.out_rec_off, B.z.stream); B.dev.download(len, B.mo.out_rec_len, B.z.stream); B.dev.download(mpos, B.mo.out_mpos, B.z.stream);
        ck(plat_stream_sync(B.z.ctx, B.z.stream), "plat_stream_sync");
    }
    // per unit: its streams' records lie back to back; ordered by mate position, equal positions in fetch order
    for (size_t s0 = 0; s0 < streams.size();) {
        size_t s1 = s0;
        while (s1 < streams.size() && streams[s1].k == streams[s0].k && streams[s1].f == streams[s0].f) ++s1;
        const size_t u = (size_t)streams[s0].k * n_files + streams[s0].f, r0 = (size_t)B.outBegin[s0], r1 = (size_t)B.outBegin[s1];
        if (r1 > r0) {
            std::vector<size_t> order(r1 - r0);
            for (size_t i = 0; i < order.size(); ++i) order[i] = r0 + i;
            std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return mpos[a] < mpos[b]; });
            const int64_t base = off[r0], bytes = off[r1 - 1] + len[r1 - 1] - base;
            plat_bam_records& r = I.M[u].mates.records;
            r.data = I.blob.data() + base; r.data_len = bytes;
            for (size_t i : order) { I.recOff[u].push_back(off[i] - base); I.recLen[u].push_back(len[i]); }
        }
        s0 = s1;
    }
    return publish();
}

}  // namespace plathost

CALLER_EXPORT int plat_bam_files_mates_plan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                                            const plat_bam_fetch_plan* fetch_plan, const plat_caller_options* options, plat_bam_mates_plan** plan)
{
    return bamFilesPlanEntry<plat_bam_mates_plan_impl>("plat_bam_files_mates_plan", plan, files, n_files, regions, n_regions, fetch_plan && options, [&](plat_bam_mates_plan_impl& I) {
        return makeBamMatesPlan(files, n_files, regions, n_regions, *fetch_plan, *options, I);
    });
}
CALLER_EXPORT void plat_bam_mates_plan_free(plat_bam_mates_plan* plan) { delete static_cast<plat_bam_mates_plan_impl*>(plan); }

CALLER_EXPORT int plat_call_bam_files_mates(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                                            plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                            plat_fetched_region_info* info, plat_caller_stats* stats)
{
    if (!options || !(options->assemble && options->assembleBrokenPairs))  // (the reference fetches no mates: the call is plat_call_bam_files)
        return plat_call_bam_files(c, files, n_files, regions, n_regions, options, qc, out_text, out_len, info, stats);
    if (!bamFilesCallArgsOk(c, files, n_files, regions, n_regions, options, out_text, out_len)) return PLAT_ERR_INVALID;
    SourceLinesGuard sourceGuard(c);                                       // (whichever way this call ends; the BGZF call behind it holds its own)
    const int rc = needsEntryPoints(c, "plat_call_bam_files_mates", {(const void*)plat_bam_mates_batch}, "plat_bam_mates_batch");
    if (rc != PLAT_OK) return rc;
    plat_bam_mates_plan_impl MP;
    return callBamFilesWith(c, "plat_call_bam_files_mates", files, n_files, regions, n_regions, options, qc, out_text, out_len, info, stats,
                            [&](const plat_bam_plan_impl&, const plat_bam_fetch_plan_impl& X, const plat_bam_mates** units, long long* mateBytes) {
                                const int r = guardedEntry(c, "plat_call_bam_files_mates", [&] { return makeBamMatesPlan(files, n_files, regions, n_regions, X, *options, MP); });
                                if (r == PLAT_OK) { *units = MP.M.data(); *mateBytes = MP.input_bytes; }
                                return r;
                            });
}
