// bgzf_blocks.hpp -- the BGZF blocks of one call, for every host entry point that takes compressed bytes (bgzf_regions.hpp and through it
// rg_regions.hpp, bam_mates.hpp, tabix_source.hpp, tbi_out.hpp, index_source.hpp): the walk over a chunk's BSIZE chain with its refusals
// (18 header bytes and the trailer of every block, never a payload byte), the upload and plat_bgzf_inflate_batch on the device, the same
// inflate on the host (bgzf::inflate_block), and the message for a block either of them refused (BgzfBlockList); and, for the callers that
// fetch BAM records, the batch from such a list to the kept records' offsets on the device (BgzfStreams: the inflate,
// plat_bam_find_records over the caller's streams, the two status blocks and their messages).  Neither knows which front end it serves:
// the entry point's name and the words for a chunk's or a stream's place are the caller's, and errors go to the string the caller hands over.
// The block list without inflateOnDevice needs csrc/bgzf_inflate.hpp, plat_bgzf_chunk and the standard library alone.
// PLAT_BGZF_BLOCKS_HOST_ONLY: without inflateOnDevice and BgzfStreams, for a stand-alone program (tests/bgzf_blocks_driver.cpp and the tabix
// drivers run this walk under the sanitizers).  With them: included behind front_end.hpp (Slot, FetchedDeviceBuffers, RecordList).
#pragma once
#include <climits>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "../../../include/platypus_mi355x.h"
#include "../../../include/platypus_caller_bgzf.h"
#include "../bgzf_inflate.hpp"

#ifndef PLAT_BGZF_BLOCKS_HOST_ONLY
// referenced weakly, as plat_bam_decode_batch: the CPU suite's stand-in device library predates them
#pragma weak plat_bgzf_inflate_batch
#pragma weak plat_bam_find_records
#endif

namespace plathost {

struct BgzfChunkAt { int region, unit, chunk, blkFirst, blkEnd; };        // where a chunk came from and its blocks in the call's list

// what every entry point checks of a chunk before it reads its data
inline bool bgzfChunkArgsOk(const plat_bgzf_chunk& ch) {
    return !(ch.data_len < 0 || (ch.data_len && !ch.data) || ch.first_uoffset < 0 || ch.first_uoffset > 65535 || ch.end_uoffset < 0 || ch.end_uoffset > 65536 ||
             ch.end_coffset < -1 || ch.end_coffset > ch.data_len);
}
// The BSIZE chain of one chunk's data (18 header bytes and the trailer of every block): block(at, head) for every block in order, false
// ends the walk.  Returns -1 when the chain covers the data, -2 when block() ended it, else the offset at which no valid header stands.
template <class Block> inline int64_t walkBgzfChain(const plat_bgzf_chunk& ch, Block&& block) {
    for (int64_t at = 0; at < ch.data_len;) {
        bgzf::BlockHead h;
        if (bgzf::parse_header(ch.data, ch.data_len, at, &h) != 0) return at;
        if (!block(at, h)) return -2;
        at = h.payload + h.payload_len + 8;
    }
    return -1;
}

// The chunks of one call in order, each a run of whole blocks, and the blocks of all of them as plat_bgzf_inflate_batch takes them.
struct BgzfBlockList {
    const std::string entry;                                              // the entry point's name, in front of every message
    const std::function<std::string(const BgzfChunkAt&)> place;           // "region K, file F, chunk Q"; "": the chunk is a whole file
    const bool refuseEmpty;                                               // an empty block with data behind it ends a tabix reader: refused (BAM readers go on)
    std::string& error;
    std::vector<BgzfChunkAt> chunkAt;
    std::vector<const plat_bgzf_chunk*> chunkOf;
    std::vector<int32_t> firstU, stopBlk, stopU;                          // per chunk: where its bytes start; the block and offset at which they stop (-1: at its end)
    std::vector<int64_t> blkOff, blkLimit, blkInflated;                   // per block: where it lies in the call's blob and where its chunk ends there; the inflated bytes in front of it
    long long blobBytes = 0, inflated = 0;

    BgzfBlockList(const std::string& entry_, std::function<std::string(const BgzfChunkAt&)> place_, bool refuse_empty, std::string& error_)
        : entry(entry_), place(std::move(place_)), refuseEmpty(refuse_empty), error(error_) {}

    int nBlocks() const { return (int)blkOff.size(); }
    int64_t inflatedEnd(int b) const { return b + 1 < nBlocks() ? blkInflated[(size_t)b + 1] : (int64_t)inflated; }      // where block b's inflated bytes end

    // chunk q of unit i of region k: its fields checked, its BSIZE chain walked, end_coffset found among the block starts
    int add(int k, int i, int q, const plat_bgzf_chunk& ch)
    {
        if (!bgzfChunkArgsOk(ch)) return PLAT_ERR_INVALID;
        BgzfChunkAt a{k, i, q, nBlocks(), 0};
        int endBlk = ch.end_coffset < 0 || (ch.end_coffset == ch.data_len && ch.end_uoffset == 0) ? -1 : -2;       // -2: not found yet
        int emptyBlk = -1, emptyInFront = -1;                             // the first block of a trailing run of empty ones; an empty one with bytes behind it
        const int64_t broke = walkBgzfChain(ch, [&](int64_t at, const bgzf::BlockHead& h) {
            const int b = nBlocks();
            if (at == ch.end_coffset) endBlk = b;
            if (h.isize == 0) { if (emptyBlk < 0) emptyBlk = b; }
            else { if (emptyBlk >= 0 && emptyInFront < 0) emptyInFront = emptyBlk; emptyBlk = -1; }
            blkOff.push_back(blobBytes + at); blkLimit.push_back(blobBytes + ch.data_len); blkInflated.push_back(inflated);
            inflated += h.isize;
            return blkOff.size() < (size_t)INT_MAX;
        });
        const std::string where = broke == -1 && !(refuseEmpty && emptyInFront >= 0) && endBlk != -2 ? std::string() : place(a);      // (a message needs it)
        if (broke == -2) { error = entry + ": more blocks than one call takes"; return PLAT_ERR_OVERFLOW; }
        if (broke >= 0) {
            error = entry + (where.empty() ? ": the file's BGZF blocks" : ": the BGZF blocks of " + where) + " do not chain: no valid block header at offset " +
                    std::to_string(broke) + (where.empty() ? " (bad magic, no BC subfield, or a block that leaves the file)"
                                                           : " of its data (bad magic, no BC subfield, or a block that leaves the data)");
            return PLAT_ERR_BAD_INPUT;
        }
        if (refuseEmpty && emptyInFront >= 0) {
            error = entry + ": block " + std::to_string(emptyInFront - a.blkFirst) + (where.empty() ? "" : " of " + where) + " is empty (ISIZE 0) with data behind it: tabix ends " +
                    (where.empty() ? "the file there" : "a fetch, or cuts a line, there");
            return PLAT_ERR_BAD_INPUT;
        }
        if (endBlk == -2) {
            error = entry + ": end_coffset " + std::to_string(ch.end_coffset) + " of " + where + " is not a block boundary of its data";
            return PLAT_ERR_BAD_INPUT;
        }
        a.blkEnd = nBlocks();
        chunkAt.push_back(a); chunkOf.push_back(&ch);
        firstU.push_back(ch.first_uoffset); stopBlk.push_back(endBlk); stopU.push_back(endBlk < 0 ? 0 : ch.end_uoffset);
        blobBytes += ch.data_len;
        return PLAT_OK;
    }

    // chunk q in the call's inflated bytes: where its lines or records start, where they stop, where its bytes end
    void span(size_t q, int64_t& first, int64_t& stop, int64_t& hi) const
    {
        auto offOf = [&](int b) { return b < nBlocks() ? blkInflated[(size_t)b] : (int64_t)inflated; };
        const int64_t lo = offOf(chunkAt[q].blkFirst), e = stopBlk[q] < 0 ? offOf(chunkAt[q].blkEnd) : offOf(stopBlk[q]) + stopU[q];
        hi = offOf(chunkAt[q].blkEnd);
        first = lo + firstU[q]; stop = e < lo ? lo : e > hi ? hi : e;
    }

    // Every block inflated by the scalar driver, out[0, inflated) written: the first block that does not inflate to its ISIZE bytes, or -1.
    int64_t inflateOnHost(uint8_t* out) const
    {
        uint32_t crcTable[256];
        for (uint32_t i = 0; i < 256; ++i) crcTable[i] = bgzf::crc_table_entry(i);
        std::unique_ptr<bgzf::Tables> tables(new bgzf::Tables);
        long long base = 0;
        for (size_t q = 0; q < chunkAt.size(); base += chunkOf[q]->data_len, ++q)
            for (int b = chunkAt[q].blkFirst; b < chunkAt[q].blkEnd; ++b) {
                const int64_t room = inflatedEnd(b) - blkInflated[(size_t)b];
                if (bgzf::inflate_block(chunkOf[q]->data, chunkOf[q]->data_len, blkOff[(size_t)b] - base, out + blkInflated[(size_t)b], room, *tables, crcTable) != room) return b;
            }
        return -1;
    }
    // ... into `data`, made inflated + pad zero bytes
    int64_t inflateOnHost(std::vector<uint8_t>& data, size_t pad = 0) const { data.assign((size_t)inflated + pad, 0); return inflateOnHost(data.data()); }

    // the message for block b, refused by either inflate (PLAT_ERR_OVERFLOW: the device's words for too little room); returns the code
    int blockRefused(long long b, int code) const
    {
        size_t q = 0;
        while (q + 1 < chunkAt.size() && !(b >= chunkAt[q].blkFirst && b < chunkAt[q].blkEnd)) ++q;
        const BgzfChunkAt a = chunkAt.empty() ? BgzfChunkAt{0, 0, 0, 0, 0} : chunkAt[q];
        const std::string where = place(a);
        error = entry + ": block " + std::to_string(b - a.blkFirst) + (where.empty() ? "" : " of " + where) +
                (code == PLAT_ERR_OVERFLOW ? " does not fit the room its ISIZE words asked for"
                                           : " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)");
        return code;
    }

#ifndef PLAT_BGZF_BLOCKS_HOST_ONLY
    // Upload (chunk by chunk from the caller's memory) and inflate, back to back on the slot's stream; limits: every block held inside its
    // own chunk; upload: the copy's name in a device error.  The status block stays on the device: the caller queues its copy in front of its one wait.
    plat_bgzf_inflate_out inflateOnDevice(Slot& z, FetchedDeviceBuffers& dev, bool limits = true, const char* upload = "plat_memcpy_h2d(blocks)") const
    {
        void* st = z.stream;
        uint8_t* dBlob = dev.alloc<uint8_t>((size_t)blobBytes);
        { long long base = 0;
          for (const plat_bgzf_chunk* ch : chunkOf) {
              if (ch->data_len) ck(plat_memcpy_h2d(z.ctx, dBlob + base, ch->data, (size_t)ch->data_len, st), upload);
              base += ch->data_len;
          } }
        plat_bgzf_inflate_out io;
        memset(&io, 0, sizeof io);
        io.cap_bytes = inflated;
        io.data = dev.alloc<uint8_t>((size_t)inflated + PLAT_BLOB_PAD); io.out_off = dev.alloc<int64_t>((size_t)nBlocks() + 1); io.status = dev.alloc<int64_t>(4);
        const int64_t* dOff = dev.upload(blkOff, st);
        ck(plat_bgzf_inflate_batch(z.ctx, nBlocks(), dBlob, blobBytes, dOff, limits ? dev.upload(blkLimit, st) : nullptr, &io, st), "plat_bgzf_inflate_batch");
        return io;
    }
#endif
};

#ifndef PLAT_BGZF_BLOCKS_HOST_ONLY
// one stream of the record walk: chunks [chunkBegin, chunkEnd) of the batch's list, walked in order for the records of tid:[beg, end)
struct BgzfStream { int chunkBegin, chunkEnd; int32_t tid, beg, end; };

// One batch from chunks to kept records on a slot's stream, for every caller that fetches BAM records (BgzfFront, bgzf_regions.hpp;
// MatesBatch, bam_mates.hpp): the block list, the upload and the inflate, plat_bam_find_records (sam_itr_next) over whatever streams the
// caller lays over the list's chunks, and the messages of the two status blocks.  Nothing here waits: the statuses and the streams' begins
// are on their way back when inflate() and find() return, and firstFailure() reads them behind the caller's one wait.
struct BgzfStreams {
    Slot& z;
    FetchedDeviceBuffers& dev;
    BgzfBlockList L;
    plat_bgzf_inflate_out io;
    plat_bam_find_out fo;
    long long capRecords = 0;
    int64_t inflateStatus[4] = {0, -1, 0, 0}, findStatus[4] = {0, -1, 0, 0};

    BgzfStreams(Slot& z_, FetchedDeviceBuffers& dev_, const std::string& entry, std::function<std::string(const BgzfChunkAt&)> place, std::string& error)
        : z(z_), dev(dev_), L(entry, std::move(place), false, error) { memset(&io, 0, sizeof io); memset(&fo, 0, sizeof fo); }

    // room for the find: every record has a block_size word and 32 fixed bytes
    long long recordCap() const { return L.inflated / 36 + 1; }

    // upload and inflate, back to back; room for the find's records
    void inflate()
    {
        io = L.inflateOnDevice(z, dev);
        capRecords = recordCap();
        memset(&fo, 0, sizeof fo);
        fo.cap_records = capRecords; fo.rec_off = dev.alloc<int64_t>((size_t)capRecords); fo.rec_limit = dev.alloc<int64_t>((size_t)capRecords);
        fo.status = dev.alloc<int64_t>(4);
        dev.download(inflateStatus, io.status, 4, z.stream);
    }

    // the find over `streams`: the kept records where the decode, the route and the mates pass take them, their counts per stream
    void find(const std::vector<BgzfStream>& streams, RecordList& kept)
    {
        void* st = z.stream;
        const int n = (int)streams.size();
        std::vector<int32_t> chunkBegin(1, 0), cFirst, cEnd, cFirstU, cStopBlk, cStopU, sTid, sBeg, sEnd;
        for (const BgzfStream& s : streams) {
            for (int q = s.chunkBegin; q < s.chunkEnd; ++q) {
                cFirst.push_back(L.chunkAt[(size_t)q].blkFirst); cEnd.push_back(L.chunkAt[(size_t)q].blkEnd);
                cFirstU.push_back(L.firstU[(size_t)q]); cStopBlk.push_back(L.stopBlk[(size_t)q]); cStopU.push_back(L.stopU[(size_t)q]);
            }
            chunkBegin.push_back((int32_t)cFirst.size());
            sTid.push_back(s.tid); sBeg.push_back(s.beg); sEnd.push_back(s.end);
        }
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

    // behind the wait: 0, or the inflate's or the find's error with its message (whereStream(s): the words for stream s of the last find)
    template <class Where> int firstFailure(Where&& whereStream) const
    {
        if (inflateStatus[0] != 0) return L.blockRefused(inflateStatus[1], (int)inflateStatus[0]);
        if (findStatus[0] != 0) {
            L.error = L.entry + ": the record walk of " + whereStream((int)findStatus[1]) + " fails (a block_size below 32, or a record or its CIGAR running past the chunk's bytes)";
            return (int)findStatus[0];
        }
        return PLAT_OK;
    }
};
#endif

}  // namespace plathost
