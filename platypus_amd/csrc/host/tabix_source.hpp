// tabix_source.hpp -- plat_caller_set_source_blocks (include/platypus_caller_tabix.h): source VCFs as the BGZF blocks of their tabix fetches.
// The chunks' compressed bytes go to the device as they are, plat_bgzf_inflate_batch inflates them, plat_tabix_fetch_batch is ti_iter_read
// (the rule: tabix_rule.hpp), and the kept lines alone come back: from there on the call is plat_caller_set_source_lines with text the
// caller object owns.  The host reads each block's header and trailer (bgzf_regions.hpp's chain walk) and never a payload byte --
// unless PLAT_CALLER_HOST_TABIX=1 asks it to inflate (bgzf::inflate_block) and walk (tbxrule::walk_stream) itself.
// Included at the end of region_caller.cpp, after bgzf_regions.hpp.
#pragma once
#include "../../../include/platypus_caller_tabix.h"
#include "../tabix_rule.hpp"

// referenced weakly, as plat_bgzf_inflate_batch (bgzf_regions.hpp): the CPU suite's stand-in device library predates it
#pragma weak plat_tabix_fetch_batch

namespace plathost {

// The fetches of one call -- every (region, file) in order is one stream -- from the host's walk over the block headers to the kept text.
struct TabixSource {
    plat_caller* c;
    const std::string entry = "plat_caller_set_source_blocks";
    struct ChunkAt { int region, file, chunk, blkFirst, blkEnd; };
    std::vector<ChunkAt> chunkAt;
    std::vector<const plat_bgzf_chunk*> chunkOf;
    std::vector<int64_t> blkOff, blkLimit, blkInflated;                   // per block: where it lies in the call's blob; the inflated bytes in front of it
    std::vector<int32_t> firstU, stopBlk, stopU, chunkBegin{0}, nameOff{0}, beg, end, streamRegion, streamFile;
    std::vector<uint8_t> names;
    long long blobBytes = 0, inflated = 0;
    // what comes back
    std::vector<char> text;
    std::vector<int64_t> textOff, counts;
    int64_t fetchStatus[4] = {0, -1, 0, 0};

    explicit TabixSource(plat_caller* c_) : c(c_) {}

    std::string where(int k, int f) const { return "region " + std::to_string(k) + ", file " + std::to_string(f); }
    std::string where(const ChunkAt& a) const { return where(a.region, a.file) + ", chunk " + std::to_string(a.chunk); }

    // fetch f of region k: its chunks checked, the BSIZE chain of each walked, an empty block in front of data refused
    int add(int k, int f, const plat_tabix_fetch& ft)
    {
        if (!ft.seq_name || ft.n_chunks < 0 || (ft.n_chunks && !ft.chunks)) return PLAT_ERR_INVALID;
        for (int q = 0; q < ft.n_chunks; ++q) {
            const plat_bgzf_chunk& ch = ft.chunks[q];
            if (!bgzfChunkArgsOk(ch)) return PLAT_ERR_INVALID;
            ChunkAt a{k, f, q, (int)blkOff.size(), 0};
            int endBlk = ch.end_coffset < 0 || (ch.end_coffset == ch.data_len && ch.end_uoffset == 0) ? -1 : -2;       // -2: not found yet
            int emptyBlk = -1, emptyInFront = -1;                          // the first block of a trailing run of empty ones; an empty one with bytes behind it
            const int64_t broke = walkBgzfChain(ch, [&](int64_t at, const bgzf::BlockHead& h) {
                const int b = (int)blkOff.size();
                if (at == ch.end_coffset) endBlk = b;
                if (h.isize == 0) { if (emptyBlk < 0) emptyBlk = b; }
                else { if (emptyBlk >= 0 && emptyInFront < 0) emptyInFront = emptyBlk; emptyBlk = -1; }
                blkOff.push_back(blobBytes + at); blkLimit.push_back(blobBytes + ch.data_len); blkInflated.push_back(inflated);
                inflated += h.isize;
                return blkOff.size() < (size_t)INT_MAX;
            });
            if (broke == -2) { c->lastError = entry + ": more blocks than one call takes"; return PLAT_ERR_OVERFLOW; }
            if (broke >= 0) {
                c->lastError = entry + ": the BGZF blocks of " + where(a) + " do not chain: no valid block header at offset " + std::to_string(broke) +
                               " of its data (bad magic, no BC subfield, or a block that leaves the data)";
                return PLAT_ERR_BAD_INPUT;
            }
            if (emptyInFront >= 0) {
                c->lastError = entry + ": block " + std::to_string(emptyInFront - a.blkFirst) + " of " + where(a) +
                               " is empty (ISIZE 0) with data behind it: tabix ends a fetch, or cuts a line, there";
                return PLAT_ERR_BAD_INPUT;
            }
            if (endBlk == -2) {
                c->lastError = entry + ": end_coffset " + std::to_string(ch.end_coffset) + " of " + where(a) + " is not a block boundary of its data";
                return PLAT_ERR_BAD_INPUT;
            }
            a.blkEnd = (int)blkOff.size();
            chunkAt.push_back(a); chunkOf.push_back(&ch);
            firstU.push_back(ch.first_uoffset); stopBlk.push_back(endBlk); stopU.push_back(endBlk < 0 ? 0 : ch.end_uoffset);
            blobBytes += ch.data_len;
        }
        chunkBegin.push_back((int32_t)chunkAt.size());
        const size_t n = strlen(ft.seq_name);
        if (names.size() + n > (size_t)INT_MAX) { c->lastError = entry + ": more name bytes than one call takes"; return PLAT_ERR_OVERFLOW; }
        names.insert(names.end(), (const uint8_t*)ft.seq_name, (const uint8_t*)ft.seq_name + n);
        nameOff.push_back((int32_t)names.size());
        beg.push_back(ft.itr_beg); end.push_back(ft.itr_end); streamRegion.push_back(k); streamFile.push_back(f);
        return PLAT_OK;
    }

    int nStreams() const { return (int)beg.size(); }
    long long capText() const { return inflated + (long long)chunkAt.size(); }      // (every line ends in its chunk's bytes, one per chunk may lack its '\n')

    int blockRefused(long long b, bool overflow) {
        size_t q = 0;
        while (q + 1 < chunkAt.size() && !(b >= chunkAt[q].blkFirst && b < chunkAt[q].blkEnd)) ++q;
        const ChunkAt a = chunkAt.empty() ? ChunkAt{0, 0, 0, 0, 0} : chunkAt[q];
        c->lastError = entry + ": block " + std::to_string(b - a.blkFirst) + " of " + where(a) +
                       (overflow ? " does not fit the room its ISIZE words asked for"
                                 : " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)");
        return overflow ? PLAT_ERR_OVERFLOW : PLAT_ERR_BAD_INPUT;
    }
    int walkRefused(int s) {
        c->lastError = entry + ": the line walk of " + where(streamRegion[(size_t)s], streamFile[(size_t)s]) +
                       " fails (a line that runs past the end of a chunk that is not the fetch's last, or a POS or END beyond 32 bits)";
        return PLAT_ERR_BAD_INPUT;
    }

    // upload, inflate and fetch back to back on slot 0's stream, one wait, then the kept text
    int onDevice()
    {
        Slot& z = *c->slots[0];
        FetchedDeviceBuffers dev;
        dev.ctx = z.ctx;
        void* st = z.stream;
        const int nBlocks = (int)blkOff.size(), n = nStreams();
        uint8_t* dBlob = dev.alloc<uint8_t>((size_t)blobBytes);
        { long long base = 0;
          for (const plat_bgzf_chunk* ch : chunkOf) {
              if (ch->data_len) ck(plat_memcpy_h2d(z.ctx, dBlob + base, ch->data, (size_t)ch->data_len, st), "plat_memcpy_h2d(blocks)");
              base += ch->data_len;
          } }
        plat_bgzf_inflate_out io;
        memset(&io, 0, sizeof io);
        io.cap_bytes = inflated;
        io.data = dev.alloc<uint8_t>((size_t)inflated + PLAT_BLOB_PAD); io.out_off = dev.alloc<int64_t>((size_t)nBlocks + 1); io.status = dev.alloc<int64_t>(4);
        ck(plat_bgzf_inflate_batch(z.ctx, nBlocks, dBlob, blobBytes, dev.upload(blkOff, st), dev.upload(blkLimit, st), &io, st), "plat_bgzf_inflate_batch");
        plat_tabix_fetch_in fi;
        memset(&fi, 0, sizeof fi);
        fi.n_streams = n; fi.n_chunks = (int)chunkAt.size(); fi.n_blocks = nBlocks; fi.data = io.data; fi.data_len = inflated; fi.out_off = io.out_off;
        std::vector<int32_t> cFirst, cEnd;
        for (const ChunkAt& a : chunkAt) { cFirst.push_back(a.blkFirst); cEnd.push_back(a.blkEnd); }
        fi.stream_chunk_begin = dev.upload(chunkBegin, st);
        fi.chunk_blk_first = dev.upload(cFirst, st); fi.chunk_blk_end = dev.upload(cEnd, st); fi.chunk_first_uoffset = dev.upload(firstU, st);
        fi.chunk_stop_blk = dev.upload(stopBlk, st); fi.chunk_stop_uoffset = dev.upload(stopU, st);
        fi.names = dev.upload(names, st); fi.name_off = dev.upload(nameOff, st); fi.beg = dev.upload(beg, st); fi.end = dev.upload(end, st);
        plat_tabix_fetch_out fo;
        memset(&fo, 0, sizeof fo);
        fo.cap_text = capText();
        fo.text = dev.alloc<uint8_t>((size_t)fo.cap_text + PLAT_BLOB_PAD); fo.stream_text_off = dev.alloc<int64_t>((size_t)n + 1);
        fo.stream_counts = dev.alloc<int64_t>(2 * (size_t)n); fo.status = dev.alloc<int64_t>(4);
        ck(plat_tabix_fetch_batch(z.ctx, &fi, &fo, st), "plat_tabix_fetch_batch");
        int64_t inflateStatus[4] = {0, -1, 0, 0};
        textOff.assign((size_t)n + 1, 0); counts.assign(2 * (size_t)n, 0);
        ck(plat_memcpy_d2h(z.ctx, inflateStatus, io.status, sizeof inflateStatus, st), "plat_memcpy_d2h");
        ck(plat_memcpy_d2h(z.ctx, fetchStatus, fo.status, sizeof fetchStatus, st), "plat_memcpy_d2h");
        ck(plat_memcpy_d2h(z.ctx, textOff.data(), fo.stream_text_off, textOff.size() * sizeof(int64_t), st), "plat_memcpy_d2h");
        if (n) ck(plat_memcpy_d2h(z.ctx, counts.data(), fo.stream_counts, counts.size() * sizeof(int64_t), st), "plat_memcpy_d2h");
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        if (inflateStatus[0] != 0) return blockRefused(inflateStatus[1], inflateStatus[0] == PLAT_ERR_OVERFLOW);
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
        const int nBlocks = (int)blkOff.size(), n = nStreams();
        std::vector<uint8_t> blob((size_t)blobBytes), data((size_t)inflated + PLAT_BLOB_PAD, 0);
        { long long base = 0;
          for (const plat_bgzf_chunk* ch : chunkOf) {
              if (ch->data_len) memcpy(blob.data() + base, ch->data, (size_t)ch->data_len);
              base += ch->data_len;
          } }
        uint32_t crcTable[256];
        for (uint32_t i = 0; i < 256; ++i) crcTable[i] = bgzf::crc_table_entry(i);
        std::unique_ptr<bgzf::Tables> tables(new bgzf::Tables);
        for (int b = 0; b < nBlocks; ++b) {
            const int64_t room = (b + 1 < nBlocks ? blkInflated[(size_t)b + 1] : inflated) - blkInflated[(size_t)b];
            if (bgzf::inflate_block(blob.data(), blkLimit[(size_t)b], blkOff[(size_t)b], data.data() + blkInflated[(size_t)b], room, *tables, crcTable) != room)
                return blockRefused(b, false);
        }
        auto offOf = [&](int b) { return b < nBlocks ? blkInflated[(size_t)b] : (int64_t)inflated; };
        textOff.assign(1, 0); counts.clear();
        for (int s = 0; s < n; ++s) {
            std::vector<int64_t> first, stop, hi;
            for (int q = chunkBegin[(size_t)s]; q < chunkBegin[(size_t)s + 1]; ++q) {
                const ChunkAt& a = chunkAt[(size_t)q];
                const int64_t lo = offOf(a.blkFirst), h = offOf(a.blkEnd);
                const int64_t e = stopBlk[(size_t)q] < 0 ? h : offOf(stopBlk[(size_t)q]) + stopU[(size_t)q];
                first.push_back(lo + firstU[(size_t)q]); hi.push_back(h); stop.push_back(e < lo ? lo : e > h ? h : e);
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
    if (!onHost && (!plat_bgzf_inflate_batch || !plat_tabix_fetch_batch)) {
        c->lastError = "plat_caller_set_source_blocks: the device library has no plat_tabix_fetch_batch";
        return PLAT_ERR_UNSUPPORTED;
    }
    TabixSource W(c);
    std::vector<int> firstStream((size_t)n_regions + 1, 0);
    for (int k = 0; k < n_regions; ++k) {
        for (int f = 0; f < per_region[k].n_fetches; ++f) {
            const int rc = W.add(k, f, per_region[k].fetches[f]);
            if (rc != PLAT_OK) return rc;
        }
        firstStream[(size_t)k + 1] = W.nStreams();
    }
    int rc;
    try { rc = onHost ? W.onHost() : W.onDevice(); }
    catch (const DeviceError& e) { c->lastError = e.what(); return e.code; }
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
        info->n_blocks = (int64_t)W.blkOff.size(); info->compressed_bytes = W.blobBytes; info->inflated_bytes = W.inflated;
        for (size_t s = 0; s < (size_t)W.nStreams(); ++s) { info->lines_walked += W.counts[2 * s]; info->lines_kept += W.counts[2 * s + 1]; }
        info->kept_bytes = W.fetchStatus[3];
        info->seconds = secs(t0, Clock::now());
    }
    return PLAT_OK;
}
