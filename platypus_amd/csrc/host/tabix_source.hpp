// tabix_source.hpp -- plat_caller_set_source_blocks (include/platypus_caller_tabix.h): source VCFs as the BGZF blocks of their tabix fetches.
// The chunks' compressed bytes go to the device as they are, plat_bgzf_inflate_batch inflates them, plat_tabix_fetch_batch is ti_iter_read
// (the rule: tabix_rule.hpp), and the kept lines alone come back: from there on the call is plat_caller_set_source_lines with text the
// caller object owns.  The walk over the block headers, the upload and both inflates are bgzf_blocks.hpp's; the host never reads a payload
// byte -- unless PLAT_CALLER_HOST_TABIX=1 asks it to inflate (bgzf::inflate_block) and walk (tbxrule::walk_stream) itself.
// Included at the end of region_caller.cpp, after bgzf_regions.hpp.
#pragma once
#include "../../../include/platypus_caller_tabix.h"
#include "../tabix_rule.hpp"

// referenced weakly, as plat_bgzf_inflate_batch (bgzf_blocks.hpp): the CPU suite's stand-in device library predates it
#pragma weak plat_tabix_fetch_batch

namespace plathost {

// The fetches of one call -- every (region, file) in order is one stream -- from the block list to the kept text.
struct TabixSource {
    plat_caller* c;
    const std::string entry = "plat_caller_set_source_blocks";
    BgzfBlockList L;                                                      // (an empty block in front of data is refused)
    std::vector<int32_t> chunkBegin{0}, nameOff{0}, beg, end, streamRegion, streamFile;
    std::vector<uint8_t> names;
    // what comes back
    std::vector<char> text;
    std::vector<int64_t> textOff, counts;
    int64_t fetchStatus[4] = {0, -1, 0, 0};

    explicit TabixSource(plat_caller* c_)
        : c(c_), L(entry, [](const BgzfChunkAt& a) { return where(a.region, a.unit) + ", chunk " + std::to_string(a.chunk); }, true, c_->lastError) {}

    static std::string where(int k, int f) { return "region " + std::to_string(k) + ", file " + std::to_string(f); }

    // fetch f of region k: its chunks onto the list, its name and window
    int add(int k, int f, const plat_tabix_fetch& ft)
    {
        if (!ft.seq_name || ft.n_chunks < 0 || (ft.n_chunks && !ft.chunks)) return PLAT_ERR_INVALID;
        for (int q = 0; q < ft.n_chunks; ++q) { const int rc = L.add(k, f, q, ft.chunks[q]); if (rc != PLAT_OK) return rc; }
        chunkBegin.push_back((int32_t)L.chunkAt.size());
        const size_t n = strlen(ft.seq_name);
        if (names.size() + n > (size_t)INT_MAX) { c->lastError = entry + ": more name bytes than one call takes"; return PLAT_ERR_OVERFLOW; }
        names.insert(names.end(), (const uint8_t*)ft.seq_name, (const uint8_t*)ft.seq_name + n);
        nameOff.push_back((int32_t)names.size());
        beg.push_back(ft.itr_beg); end.push_back(ft.itr_end); streamRegion.push_back(k); streamFile.push_back(f);
        return PLAT_OK;
    }

    int nStreams() const { return (int)beg.size(); }
    long long capText() const { return L.inflated + (long long)L.chunkAt.size(); }      // (every line ends in its chunk's bytes, one per chunk may lack its '\n')

    int walkRefused(int s) {
        c->lastError = entry + ": the line walk of " + where(streamRegion[(size_t)s], streamFile[(size_t)s]) +
                       " fails (a line that runs past the end of a chunk that is not the fetch's last, or a POS or END beyond 32 bits)";
        return PLAT_ERR_BAD_INPUT;
    }

    // upload, inflate and fetch back to back on slot 0's stream, one wait, then the kept text
    int onDevice()
    {
        Slot& z = *c->slots[0];
        FetchedDeviceBuffers dev(z);
        void* st = z.stream;
        const int nBlocks = L.nBlocks(), n = nStreams();
        const plat_bgzf_inflate_out io = L.inflateOnDevice(z, dev);
        plat_tabix_fetch_in fi;
        memset(&fi, 0, sizeof fi);
        fi.n_streams = n; fi.n_chunks = (int)L.chunkAt.size(); fi.n_blocks = nBlocks; fi.data = io.data; fi.data_len = L.inflated; fi.out_off = io.out_off;
        std::vector<int32_t> cFirst, cEnd;
        for (const BgzfChunkAt& a : L.chunkAt) { cFirst.push_back(a.blkFirst); cEnd.push_back(a.blkEnd); }
        fi.stream_chunk_begin = dev.upload(chunkBegin, st);
        fi.chunk_blk_first = dev.upload(cFirst, st); fi.chunk_blk_end = dev.upload(cEnd, st); fi.chunk_first_uoffset = dev.upload(L.firstU, st);
        fi.chunk_stop_blk = dev.upload(L.stopBlk, st); fi.chunk_stop_uoffset = dev.upload(L.stopU, st);
        fi.names = dev.upload(names, st); fi.name_off = dev.upload(nameOff, st); fi.beg = dev.upload(beg, st); fi.end = dev.upload(end, st);
        plat_tabix_fetch_out fo;
        memset(&fo, 0, sizeof fo);
        fo.cap_text = capText();
        fo.text = dev.alloc<uint8_t>((size_t)fo.cap_text + PLAT_BLOB_PAD); fo.stream_text_off = dev.alloc<int64_t>((size_t)n + 1);
        fo.stream_counts = dev.alloc<int64_t>(2 * (size_t)n); fo.status = dev.alloc<int64_t>(4);
        ck(plat_tabix_fetch_batch(z.ctx, &fi, &fo, st), "plat_tabix_fetch_batch");
        int64_t inflateStatus[4] = {0, -1, 0, 0};
        textOff.assign((size_t)n + 1, 0); counts.assign(2 * (size_t)n, 0);
        dev.download(inflateStatus, io.status, 4, st);
        dev.download(fetchStatus, fo.status, 4, st);
        dev.download(textOff, fo.stream_text_off, st);
        dev.download(counts, fo.stream_counts, st);
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        if (inflateStatus[0] != 0) return L.blockRefused(inflateStatus[1], inflateStatus[0] == PLAT_ERR_OVERFLOW ? PLAT_ERR_OVERFLOW : PLAT_ERR_BAD_INPUT);
        if (fetchStatus[0] == PLAT_ERR_BAD_INPUT) return walkRefused((int)fetchStatus[1]);
        if (fetchStatus[0] != 0) throw DeviceError((int)fetchStatus[0], "plat_tabix_fetch_batch");
        text.resize((size_t)fetchStatus[3]);
        if (!text.empty()) {                                               // the kept lines alone
            ck(plat_memcpy_d2h(z.ctx, text.data(), fo.text, text.size(), st), "plat_memcpy_d2h(kept lines)");
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        }
        return PLAT_OK;
    }

    // the same on the host: every block inflated by the scalar driver, every stream walked by the rule
    int onHost()
    {
        const int n = nStreams();
        std::vector<uint8_t> data;
        const int64_t bad = L.inflateOnHost(data, PLAT_BLOB_PAD);
        if (bad >= 0) return L.blockRefused(bad, PLAT_ERR_BAD_INPUT);
        textOff.assign(1, 0); counts.clear();
        for (int s = 0; s < n; ++s) {
            std::vector<int64_t> first, stop, hi;
            for (int q = chunkBegin[(size_t)s]; q < chunkBegin[(size_t)s + 1]; ++q) {
                int64_t f, e, h;
                L.span((size_t)q, f, e, h);
                first.push_back(f); stop.push_back(e); hi.push_back(h);
            }
            int64_t walked = 0, kept = 0;
            const size_t before = text.size();
            const bool ok = tbxrule::walk_stream(data.data(), (int)first.size(), first.data(), stop.data(), hi.data(), names.data() + nameOff[(size_t)s],
                                                 nameOff[(size_t)s + 1] - nameOff[(size_t)s], beg[(size_t)s], end[(size_t)s], &walked, &kept,
                                                 [&](int64_t a, int64_t e) { text.insert(text.end(), (const char*)data.data() + a, (const char*)data.data() + e); text.push_back('\n'); });
            if (!ok) { text.resize(before); return walkRefused(s); }
            counts.push_back(walked); counts.push_back(kept);
            textOff.push_back((int64_t)text.size());
            fetchStatus[2] += kept;
        }
        fetchStatus[3] = (int64_t)text.size();
        return PLAT_OK;
    }
};

}  // namespace plathost

CALLER_EXPORT int plat_caller_set_source_blocks(plat_caller* c, const plat_source_blocks* per_region, int n_regions, int longHaps, plat_source_blocks_info* info)
{
    if (!c || n_regions < 0 || (n_regions > 0 && !per_region)) return PLAT_ERR_INVALID;
    const auto t0 = Clock::now();
    { SourceLinesGuard takeBack(c); }                                      // (whatever was set is gone, whichever way this call ends)
    if (info) memset(info, 0, sizeof *info);
    if (n_regions == 0) return PLAT_OK;
    for (int k = 0; k < n_regions; ++k) if (per_region[k].n_fetches < 0 || (per_region[k].n_fetches && !per_region[k].fetches)) return PLAT_ERR_INVALID;
    const bool onHost = Switches::read().hostTabix;
    const std::string entry = "plat_caller_set_source_blocks";
    int rc = onHost ? PLAT_OK : needsEntryPoints(c, entry, {(const void*)plat_bgzf_inflate_batch, (const void*)plat_tabix_fetch_batch}, "plat_tabix_fetch_batch");
    if (rc != PLAT_OK) return rc;
    return guardedEntry(c, entry, [&] {
        TabixSource W(c);
        std::vector<int> firstStream((size_t)n_regions + 1, 0);
        for (int k = 0; k < n_regions; ++k) {
            for (int f = 0; f < per_region[k].n_fetches; ++f) {
                const int rc = W.add(k, f, per_region[k].fetches[f]);
                if (rc != PLAT_OK) return rc;
            }
            firstStream[(size_t)k + 1] = W.nStreams();
        }
        const int rc = onHost ? W.onHost() : W.onDevice();
        if (rc != PLAT_OK) return rc;
        c->sourceText.swap(W.text);
        c->sourceLines.resize((size_t)n_regions);
        for (int k = 0; k < n_regions; ++k) {
            const int64_t a = W.textOff[(size_t)firstStream[(size_t)k]], b = W.textOff[(size_t)firstStream[(size_t)k + 1]];
            c->sourceLines[(size_t)k] = plat_source_lines{b > a ? c->sourceText.data() + a : nullptr, b - a};
        }
        c->sourceSet = true;
        c->sourceLongHaps = longHaps;
        if (info) {
            info->n_blocks = (int64_t)W.L.nBlocks(); info->compressed_bytes = W.L.blobBytes; info->inflated_bytes = W.L.inflated;
            for (size_t s = 0; s < (size_t)W.nStreams(); ++s) { info->lines_walked += W.counts[2 * s]; info->lines_kept += W.counts[2 * s + 1]; }
            info->kept_bytes = W.fetchStatus[3];
            info->seconds = secs(t0, Clock::now());
        }
        return (int)PLAT_OK;
    });
}
