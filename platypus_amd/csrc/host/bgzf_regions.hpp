// bgzf_regions.hpp -- plat_call_bgzf_regions (include/platypus_caller_bgzf.h): the region loop for the BGZF blocks of an index lookup.  A
// front end on front_end.hpp's frame, in front of bam_regions.hpp's decode: the chunks' compressed bytes go to the device as they are,
// plat_bgzf_inflate_batch inflates them and plat_bam_find_records is sam_itr_next (bgzf_blocks.hpp's BgzfStreams: the walk over the block
// headers, the upload, the inflate, the find and their refusals), plat_bam_decode_batch takes the kept records' offsets where the find left
// them (a RecordList), and decodeAndStage does the rest.  The host never reads a payload byte.
// Included at the end of region_caller.cpp, after bam_regions.hpp and bgzf_blocks.hpp.
#pragma once
#include "../../../include/platypus_caller_bgzf.h"

namespace plathost {

// The chunks of one call -- every (region, unit) in order, a unit being what one index lookup fetched (a sample; a file for the read-group
// call of rg_regions.hpp) -- on a BgzfStreams batch: which regions' units are the find's streams, and loadBAMData's bail-out between two finds.
struct BgzfFront {
    FrontCall& F;
    const int nUnits;
    const char* const unit;                                               // what the messages call one: "sample" or "file"
    BgzfStreams batch;                                                    // the call's blocks and chunks, all regions: which of them load is known once the device has counted the kept records
    std::vector<int32_t> tid, beg, end;                                   // per region
    std::vector<int> unitEnd;                                             // per (region, unit): where its chunks end in the batch's list (they begin where the unit in front ends)

    BgzfFront(FrontCall& f, int n_units, const char* unit_)
        : F(f), nUnits(n_units), unit(unit_),
          batch(*f.z, f.dev, f.entry, [this](const BgzfChunkAt& a) { return F.where(a.region, a.unit, unit) + ", chunk " + std::to_string(a.chunk); }, f.c->lastError) {}

    void addRegion(int32_t t, int32_t b, int32_t e) { tid.push_back(t); beg.push_back(b); end.push_back(e); }

    // unit i of region k (every unit of every region, in order): its chunks onto the list
    int addUnit(int k, int i, int n_chunks, const plat_bgzf_chunk* chunks)
    {
        for (int q = 0; q < n_chunks; ++q) { const int rc = batch.L.add(k, i, q, chunks[q]); if (rc != PLAT_OK) return rc; }
        unitEnd.push_back((int)batch.L.chunkAt.size());
        return PLAT_OK;
    }

    // the find over the streams of the regions `use` marks (stream = unit i of such a region, in order)
    void find(const std::vector<int>& use, RecordList& kept)
    {
        std::vector<BgzfStream> streams;
        if (unitEnd.size() != use.size() * (size_t)nUnits) throw DeviceError(PLAT_ERR_INVALID, F.entry + ": the find before every unit of every region was added");
        for (size_t u = 0; u < unitEnd.size(); ++u) {
            const size_t k = u / (size_t)nUnits;
            if (use[k]) streams.push_back(BgzfStream{u ? unitEnd[u - 1] : 0, unitEnd[u], tid[k], beg[k], end[k]});
        }
        batch.find(streams, kept);
    }

    // The find over every region, whatever `behind` enqueues behind it (the read-group call's routes), and the one wait in front of the
    // decode: two status blocks and the kept counts.  Then loadBAMData's bail-out on those counts; when it drops a region, the find and
    // `behind` once more over the loaded regions alone, so that their kept records lie back to back.
    template <class Behind> int findLoaded(RecordList& kept, Behind&& behind)
    {
        Slot& z = *F.z;
        std::vector<int>& loaded = F.S.loaded;
        const std::vector<int> all(loaded.size(), 1);
        find(all, kept);
        behind(all);
        ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");
        const int rc = batch.firstFailure([&](int s) { return F.where(s / nUnits, s % nUnits, unit); });      // (every region took part)
        if (rc != PLAT_OK) return rc;
        bool dropped = false;
        for (size_t k = 0; k < loaded.size(); ++k) {
            loaded[k] = !F.drops((long long)kept.begin[(k + 1) * (size_t)nUnits] - kept.begin[k * (size_t)nUnits]);
            dropped = dropped || !loaded[k];
        }
        if (!dropped) return PLAT_OK;
        find(loaded, kept);
        behind(loaded);
        ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");
        if (batch.findStatus[0] != 0) { F.c->lastError = F.entry + ": the record walk fails on its second run"; return (int)batch.findStatus[0]; }
        return PLAT_OK;
    }

    long long loadedBytes(const std::vector<int>& loaded) const {
        const BgzfBlockList& L = batch.L;
        long long b = 0;
        for (size_t q = 0; q < L.chunkAt.size(); ++q) if (loaded[(size_t)L.chunkAt[q].region]) b += L.chunkOf[q]->data_len;
        return b;
    }
};

}  // namespace plathost

CALLER_EXPORT int plat_call_bgzf_regions(plat_caller* c, const plat_bgzf_region* regions, int n_regions, int n_samples,
                                         const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                                         char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats)
{
    FrontCall F(c, "plat_call_bgzf_regions", n_regions, n_samples, sample_names, options, qc, out_text, out_len, info, stats);
    int rc = F.open(regions, true, {(const void*)plat_bgzf_inflate_batch, (const void*)plat_bam_find_records, (const void*)plat_bam_decode_batch,
                                    (const void*)plat_read_buffers_batch}, "plat_bgzf_inflate_batch");
    if (rc != PLAT_OK) return rc;
    FetchedStage& S = F.S;
    return F.guarded([&] {
        BgzfFront W(F, n_samples, "sample");
        int rc;
        for (int k = 0; k < n_regions; ++k) {
            const plat_bgzf_region& r = regions[k];
            if (!r.samples) return PLAT_ERR_INVALID;
            W.addRegion(r.tid, r.itr_beg, r.itr_end);
            for (int i = 0; i < n_samples; ++i) {
                const plat_bgzf_sample& sm = r.samples[i];
                if (sm.n_chunks < 0 || (sm.n_chunks && !sm.chunks) || !recordsValid(sm.broken_mates)) return PLAT_ERR_INVALID;
                if ((rc = W.addUnit(k, i, sm.n_chunks, sm.chunks)) != PLAT_OK) return rc;
            }
        }
        W.batch.inflate();                                                 // upload, inflate, find: back to back
        RecordList kept;
        rc = W.findLoaded(kept, [](const std::vector<int>&) {});
        if (rc != PLAT_OK) return rc;
        std::vector<const plat_bam_records*> broken;
        long long nBroken = 0;
        S.linkBytes += W.loadedBytes(S.loaded);
        for (int k = 0; k < n_regions; ++k)
            for (int i = 0; i < n_samples && S.loaded[(size_t)k]; ++i) {
                const plat_bam_records* t = &regions[k].samples[i].broken_mates;
                broken.push_back(t); nBroken += t->n_records;
                S.linkBytes += t->n_records ? t->data_len : 0;
            }
        if ((rc = F.tooMany(kept.n(), nBroken, (long long)broken.size())) != PLAT_OK) return rc;
        return decodeAndStage(F, kept, [&] { return uploadRecords(*F.z, F.dev, broken); });
    });
}
