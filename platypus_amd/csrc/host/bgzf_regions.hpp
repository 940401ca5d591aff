// bgzf_regions.hpp -- plat_call_bgzf_regions (include/platypus_caller_bgzf.h): the region loop for the BGZF blocks of an index lookup.  A
// front end on front_end.hpp's frame, in front of bam_regions.hpp's decode: the chunks' compressed bytes go to the device as they are,
// plat_bgzf_inflate_batch inflates them (bgzf_blocks.hpp: the walk over the block headers, the upload and the inflate), plat_bam_find_records
// is sam_itr_next, plat_bam_decode_batch takes the kept records' offsets where the find left them (a RecordList), and decodeAndStage does
// the rest.  The host never reads a payload byte.
// Included at the end of region_caller.cpp, after bam_regions.hpp and bgzf_blocks.hpp.
#pragma once
#include "../../../include/platypus_caller_bgzf.h"

// referenced weakly, as plat_bam_decode_batch: the CPU suite's stand-in device library predates it
#pragma weak plat_bam_find_records

namespace plathost {

// The chunks of one call -- every (region, unit) in order, a unit being what one index lookup fetched (a sample; a file for the read-group
// call of rg_regions.hpp) -- from the block list to the kept records' offsets on the device.
struct BgzfFront {
    FrontCall& F;
    const std::string& entry;
    const int nUnits;
    const char* const unit;                                               // what the messages call one: "sample" or "file"
    BgzfBlockList L;                                                      // the call's blocks and chunks, all regions: which of them load is known once the device has counted the kept records
    std::vector<int32_t> tid, beg, end;                                   // per region
    plat_bgzf_inflate_out io;
    plat_bam_find_out fo;
    long long capRecords = 0;
    int64_t inflateStatus[4] = {0, -1, 0, 0}, findStatus[4] = {0, -1, 0, 0};

    BgzfFront(FrontCall& f, int n_units, const char* unit_)
        : F(f), entry(f.entry), nUnits(n_units), unit(unit_),
          L(f.entry, [this](const BgzfChunkAt& a) { return F.where(a.region, a.unit, unit) + ", chunk " + std::to_string(a.chunk); }, false, f.c->lastError) {}

    void addRegion(int32_t t, int32_t b, int32_t e) { tid.push_back(t); beg.push_back(b); end.push_back(e); }

    // unit i of region k: its chunks onto the list
    int addUnit(int k, int i, int n_chunks, const plat_bgzf_chunk* chunks)
    {
        for (int q = 0; q < n_chunks; ++q) { const int rc = L.add(k, i, q, chunks[q]); if (rc != PLAT_OK) return rc; }
        return PLAT_OK;
    }

    // upload and inflate, back to back; room for the find's records
    void inflate()
    {
        FetchedDeviceBuffers& dev = F.dev;
        io = L.inflateOnDevice(*F.z, dev);
        // every record has a block_size word and 32 fixed bytes
        capRecords = L.inflated / 36 + 1;
        memset(&fo, 0, sizeof fo);
        fo.cap_records = capRecords; fo.rec_off = dev.alloc<int64_t>((size_t)capRecords); fo.rec_limit = dev.alloc<int64_t>((size_t)capRecords);
        fo.status = dev.alloc<int64_t>(4);
        dev.download(inflateStatus, io.status, 4, F.z->stream);
    }

    // the find over the streams of the regions `use` marks (stream = unit i of such a region, in order; its chunks lie back to back in the
    // call's list): the kept records, their counts per stream on their way back
    void find(const std::vector<int>& use, RecordList& kept)
    {
        Slot& z = *F.z;
        FetchedDeviceBuffers& dev = F.dev;
        void* st = z.stream;
        const int n_regions = (int)use.size();
        std::vector<int32_t> chunkBegin(1, 0), cFirst, cEnd, cFirstU, cStopBlk, cStopU, sTid, sBeg, sEnd;
        size_t q = 0;
        for (int k = 0; k < n_regions; ++k)
            for (int i = 0; i < nUnits; ++i) {
                for (; q < L.chunkAt.size() && L.chunkAt[q].region == k && L.chunkAt[q].unit == i; ++q) {
                    if (!use[(size_t)k]) continue;
                    cFirst.push_back(L.chunkAt[q].blkFirst); cEnd.push_back(L.chunkAt[q].blkEnd);
                    cFirstU.push_back(L.firstU[q]); cStopBlk.push_back(L.stopBlk[q]); cStopU.push_back(L.stopU[q]);
                }
                if (!use[(size_t)k]) continue;
                chunkBegin.push_back((int32_t)cFirst.size());
                sTid.push_back(tid[(size_t)k]); sBeg.push_back(beg[(size_t)k]); sEnd.push_back(end[(size_t)k]);
            }
        const int n = (int)sTid.size();
        plat_bam_find_in fi;
        memset(&fi, 0, sizeof fi);
        fi.n_streams = n; fi.n_chunks = (int)cFirst.size(); fi.n_blocks = L.nBlocks(); fi.data = io.data; fi.out_off = io.out_off;
        fi.chunk_blk_first = dev.upload(cFirst, st); fi.chunk_blk_end = dev.upload(cEnd, st); fi.chunk_first_uoffset = dev.upload(cFirstU, st);
        fi.chunk_stop_blk = dev.upload(cStopBlk, st); fi.chunk_stop_uoffset = dev.upload(cStopU, st);
        fi.stream_chunk_begin = dev.upload(chunkBegin, st);
        fi.tid = dev.upload(sTid, st); fi.beg = dev.upload(sBeg, st); fi.end = dev.upload(sEnd, st);
        fo.stream_begin = dev.alloc<int32_t>((size_t)n + 1);
        ck(plat_bam_find_records(z.ctx, &fi, &fo, st), "plat_bam_find_records");
        kept.blob = io.data; kept.bytes = L.inflated; kept.off = fo.rec_off; kept.limit = fo.rec_limit; kept.dBegin = fo.stream_begin;
        kept.begin.assign((size_t)n + 1, 0);
        dev.download(kept.begin, fo.stream_begin, st);
        dev.download(findStatus, fo.status, 4, st);
    }

    // after the wait behind the first find (every region took part): 0, or the inflate's or the find's error with its message
    int firstFailure() const
    {
        if (inflateStatus[0] != 0) return L.blockRefused(inflateStatus[1], (int)inflateStatus[0]);
        if (findStatus[0] != 0) {                                          // (stream s is unit s % nUnits of region s / nUnits)
            const int s = (int)findStatus[1];
            F.c->lastError = entry + ": the record walk of " + F.where(s / nUnits, s % nUnits, unit) +
                             " fails (a block_size below 32, or a record or its CIGAR running past the chunk's bytes)";
            return (int)findStatus[0];
        }
        return PLAT_OK;
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
        const int rc = firstFailure();
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
        if (findStatus[0] != 0) { F.c->lastError = entry + ": the record walk fails on its second run"; return (int)findStatus[0]; }
        return PLAT_OK;
    }

    long long loadedBytes(const std::vector<int>& loaded) const {
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
        W.inflate();                                                       // upload, inflate, find: back to back
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
