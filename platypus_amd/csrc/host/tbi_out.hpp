// tbi_out.hpp -- plat_caller_index_bgzf (include/platypus_caller_tbi.h): the tabix index of a whole .vcf.gz.  The host walks the block
// headers (bgzf_regions.hpp's chain walk; an empty block with data behind it is refused, as tabix_source.hpp refuses it), the file goes
// up in one copy, plat_bgzf_inflate_batch and plat_tabix_index_batch run back to back on slot 0's stream, one wait for their status
// blocks, then runs, names and windows come back and tbxindex::finish (csrc/tabix_index.hpp) makes the index of them, deflated by
// bgzf::deflate_pieces.  PLAT_CALLER_HOST_TBI=1 inflates on the host and runs tbxindex::build_serial instead: the same intermediate.
// Included at the end of region_caller.cpp, after bgzf_out.hpp.
#pragma once
#include "../../../include/platypus_caller_tbi.h"
#include "../tabix_index.hpp"

// referenced weakly, as plat_bgzf_deflate_batch (bgzf_out.hpp): the CPU suite's stand-in device library predates it
#pragma weak plat_tabix_index_batch

namespace plathost {

struct TbiOut {
    plat_caller* c;
    const uint8_t* file;
    int64_t fileLen;
    const std::string entry = "plat_caller_index_bgzf";
    std::vector<int64_t> blkOff, blkInflated, blkAddr;                    // the blocks up to the last that holds data; blkAddr has the address behind it too
    int64_t allBlocks = 0, inflated = 0;
    tbxindex::Intermediate I;
    std::vector<std::string> names;
    int deviceCalls = 0;

    TbiOut(plat_caller* c_, const uint8_t* file_, size_t len) : c(c_), file(file_), fileLen((int64_t)len) {}

    int walk() {
        plat_bgzf_chunk ch;
        memset(&ch, 0, sizeof ch);
        ch.data = file; ch.data_len = fileLen; ch.end_coffset = -1;
        std::vector<int64_t> off, isize;
        const int64_t broke = walkBgzfChain(ch, [&](int64_t at, const bgzf::BlockHead& h) {
            off.push_back(at); isize.push_back(h.isize);
            return off.size() < (size_t)INT_MAX;
        });
        if (broke == -2) { c->lastError = entry + ": more blocks than one call takes"; return PLAT_ERR_OVERFLOW; }
        if (broke >= 0) {
            c->lastError = entry + ": the file's BGZF blocks do not chain: no valid block header at offset " + std::to_string(broke) +
                           " (bad magic, no BC subfield, or a block that leaves the file)";
            return PLAT_ERR_BAD_INPUT;
        }
        allBlocks = (int64_t)off.size();
        size_t nData = off.size();
        while (nData > 0 && isize[nData - 1] == 0) --nData;
        for (size_t b = 0; b < nData; ++b) {
            if (isize[b] == 0) {
                c->lastError = entry + ": block " + std::to_string(b) + " is empty (ISIZE 0) with data behind it: tabix ends the file there";
                return PLAT_ERR_BAD_INPUT;
            }
            blkOff.push_back(off[b]); blkInflated.push_back(inflated);
            inflated += isize[b];
        }
        blkAddr = blkOff;
        blkAddr.push_back(nData < off.size() ? off[nData] : fileLen);
        return PLAT_OK;
    }

    int blockRefused(long long b) {
        c->lastError = entry + ": block " + std::to_string(b) + " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)";
        return PLAT_ERR_BAD_INPUT;
    }
    // what the status block says of a file that is no index's: the message, the code
    int verdict() {
        static const char* const kinds[] = {"", "it has fewer than two columns", "its POS or END lies beyond 32 bits", "its END is negative",
                                            "its position lies below that of the record in front of it (is the file sorted?)",
                                            "its contig appeared before, with another one between (is the file sorted?)"};
        const int64_t v = I.status[tbxindex::ST_VERDICT];
        if (v == PLAT_ERR_BAD_INPUT) {
            const int64_t k = I.status[tbxindex::ST_KIND];
            c->lastError = entry + ": line " + std::to_string(I.status[tbxindex::ST_LINE]) + " cannot be indexed: " + (k >= 1 && k <= 5 ? kinds[k] : "refused");
        } else if (v == PLAT_ERR_UNSUPPORTED) c->lastError = entry + ": more than " + std::to_string(tbxindex::MAX_REF) + " contigs";
        else if (v != 0) c->lastError = entry + ": the index call failed with " + std::to_string(v);
        return (int)v;
    }

    int onDevice() {
        Slot& z = *c->slots[0];
        FetchedDeviceBuffers dev;
        dev.ctx = z.ctx;
        void* st = z.stream;
        const int nBlocks = (int)blkOff.size();
        uint8_t* dFile = dev.alloc<uint8_t>((size_t)fileLen);
        if (fileLen) ck(plat_memcpy_h2d(z.ctx, dFile, file, (size_t)fileLen, st), "plat_memcpy_h2d(file)");
        plat_bgzf_inflate_out io;
        memset(&io, 0, sizeof io);
        io.cap_bytes = inflated;
        io.data = dev.alloc<uint8_t>((size_t)inflated + PLAT_BLOB_PAD); io.out_off = dev.alloc<int64_t>((size_t)nBlocks + 1); io.status = dev.alloc<int64_t>(4);
        ck(plat_bgzf_inflate_batch(z.ctx, nBlocks, dFile, fileLen, dev.upload(blkOff, st), nullptr, &io, st), "plat_bgzf_inflate_batch");
        plat_tabix_index_in in;
        memset(&in, 0, sizeof in);
        in.n_blocks = nBlocks; in.data = io.data; in.data_len = inflated; in.out_off = io.out_off; in.blk_addr = dev.upload(blkAddr, st);
        plat_tabix_index_out o;
        memset(&o, 0, sizeof o);
        o.status = dev.alloc<int64_t>(tbxindex::ST_WORDS);
        // record text runs to some 250 bytes a line and few lines open a run: room for a run per 64 bytes at first, the counts the device names after that
        // (a file holds at most MAX_REF contigs: their tables are given whole)
        int64_t capRuns = inflated / 64 + 1024, capWindows = (int64_t)1 << 18, capNameBytes = (int64_t)1 << 20;
        const int64_t capNames = tbxindex::MAX_REF;
        int64_t inflateStatus[4] = {0, -1, 0, 0};
        for (int attempt = 0;; ++attempt) {
            o.cap_runs = capRuns; o.cap_names = capNames; o.cap_windows = capWindows; o.cap_name_bytes = capNameBytes;
            o.run_tid = dev.alloc<int32_t>((size_t)capRuns); o.run_bin = dev.alloc<int32_t>((size_t)capRuns); o.run_u = dev.alloc<int64_t>((size_t)capRuns);
            o.name_off = dev.alloc<int64_t>((size_t)capNames); o.name_len = dev.alloc<int32_t>((size_t)capNames);
            o.lin_first = dev.alloc<int64_t>((size_t)capNames + 1); o.lin = dev.alloc<int64_t>((size_t)capWindows); o.name_bytes = dev.alloc<uint8_t>((size_t)capNameBytes);
            ck(plat_tabix_index_batch(z.ctx, &in, &o, st), "plat_tabix_index_batch");
            ++deviceCalls;
            if (attempt == 0) ck(plat_memcpy_d2h(z.ctx, inflateStatus, io.status, sizeof inflateStatus, st), "plat_memcpy_d2h");
            ck(plat_memcpy_d2h(z.ctx, I.status, o.status, sizeof I.status, st), "plat_memcpy_d2h");
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
            if (inflateStatus[0] != 0) return blockRefused(inflateStatus[1]);
            if (I.status[tbxindex::ST_VERDICT] != PLAT_ERR_OVERFLOW || attempt == 1) break;
            capRuns = I.status[tbxindex::ST_RUNS]; capWindows = I.status[tbxindex::ST_WINDOWS]; capNameBytes = I.status[tbxindex::ST_NAME_BYTES];
        }
        if (I.status[tbxindex::ST_VERDICT] != 0) return verdict();
        const size_t nRuns = (size_t)I.status[tbxindex::ST_RUNS], nRef = (size_t)I.status[tbxindex::ST_CONTIGS], nWin = (size_t)I.status[tbxindex::ST_WINDOWS];
        I.runTid.resize(nRuns); I.runBin.resize(nRuns); I.runU.resize(nRuns); I.nameOff.resize(nRef); I.nameLen.resize(nRef); I.linFirst.resize(nRef + 1); I.lin.resize(nWin);
        if (nRuns) {
            ck(plat_memcpy_d2h(z.ctx, I.runTid.data(), o.run_tid, nRuns * sizeof(int32_t), st), "plat_memcpy_d2h");
            ck(plat_memcpy_d2h(z.ctx, I.runBin.data(), o.run_bin, nRuns * sizeof(int32_t), st), "plat_memcpy_d2h");
            ck(plat_memcpy_d2h(z.ctx, I.runU.data(), o.run_u, nRuns * sizeof(int64_t), st), "plat_memcpy_d2h");
        }
        if (nRef) {
            ck(plat_memcpy_d2h(z.ctx, I.nameOff.data(), o.name_off, nRef * sizeof(int64_t), st), "plat_memcpy_d2h");
            ck(plat_memcpy_d2h(z.ctx, I.nameLen.data(), o.name_len, nRef * sizeof(int32_t), st), "plat_memcpy_d2h");
        }
        ck(plat_memcpy_d2h(z.ctx, I.linFirst.data(), o.lin_first, (nRef + 1) * sizeof(int64_t), st), "plat_memcpy_d2h");
        if (nWin) ck(plat_memcpy_d2h(z.ctx, I.lin.data(), o.lin, nWin * sizeof(int64_t), st), "plat_memcpy_d2h");
        I.nameBytes.resize((size_t)I.status[tbxindex::ST_NAME_BYTES]);     // the names' bytes: the only text the host sees
        if (!I.nameBytes.empty()) ck(plat_memcpy_d2h(z.ctx, I.nameBytes.data(), o.name_bytes, I.nameBytes.size(), st), "plat_memcpy_d2h(names)");
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        { int64_t sum = 0;
          for (int32_t n : I.nameLen) { if (n < 0) { sum = -1; break; } sum += n; }
          if (sum != (int64_t)I.nameBytes.size()) throw DeviceError(PLAT_ERR_INVALID, "plat_tabix_index_batch (name lengths that do not sum to the names' bytes)"); }
        names = tbxindex::names_of(I);
        return PLAT_OK;
    }

    int onHost() {
        const int nBlocks = (int)blkOff.size();
        std::vector<uint8_t> data((size_t)inflated + PLAT_BLOB_PAD, 0);
        uint32_t crcTable[256];
        for (uint32_t i = 0; i < 256; ++i) crcTable[i] = bgzf::crc_table_entry(i);
        std::unique_ptr<bgzf::Tables> tables(new bgzf::Tables);
        std::vector<int64_t> outOff = blkInflated;
        outOff.push_back(inflated);
        for (int b = 0; b < nBlocks; ++b) {
            const int64_t room = outOff[(size_t)b + 1] - outOff[(size_t)b];
            if (bgzf::inflate_block(file, fileLen, blkOff[(size_t)b], data.data() + outOff[(size_t)b], room, *tables, crcTable) != room) return blockRefused(b);
        }
        tbxindex::build_serial(data.data(), inflated, outOff.data(), blkAddr.data(), nBlocks, I);
        if (I.status[tbxindex::ST_VERDICT] != 0) return verdict();
        names = tbxindex::names_of(I);
        return PLAT_OK;
    }
};

}  // namespace plathost

CALLER_EXPORT int plat_caller_index_bgzf(plat_caller* c, const uint8_t* file, size_t len, uint8_t** tbi, size_t* tbi_len, plat_tbi_info* info)
{
    if (!c || !tbi || !tbi_len || (len > 0 && !file)) return PLAT_ERR_INVALID;
    const auto t0 = Clock::now();
    *tbi = nullptr; *tbi_len = 0;
    if (info) { memset(info, 0, sizeof *info); info->refused_line = -1; }
    const bool onHost = Switches::read().hostTbi;
    if (!onHost && (!plat_bgzf_inflate_batch || !plat_tabix_index_batch)) {
        c->lastError = "plat_caller_index_bgzf: the device library has no plat_tabix_index_batch";
        return PLAT_ERR_UNSUPPORTED;
    }
    TbiOut W(c, file, len);
    int rc = W.walk();
    if (rc != PLAT_OK) return rc;
    try { rc = onHost ? W.onHost() : W.onDevice(); }
    catch (const DeviceError& e) { c->lastError = e.what(); return e.code; }
    catch (const std::exception& e) { c->lastError = std::string("plat_caller_index_bgzf: ") + e.what(); return PLAT_ERR_NOMEM; }
    if (info) {
        info->n_blocks = W.allBlocks; info->compressed_bytes = (int64_t)len; info->inflated_bytes = W.inflated; info->device_calls = W.deviceCalls;
        info->refused_line = W.I.status[tbxindex::ST_LINE]; info->seconds = secs(t0, Clock::now());
    }
    if (rc != PLAT_OK) return rc;
    const std::vector<uint8_t> raw = tbxindex::finish(W.I, W.names);
    std::vector<uint8_t> packed;
    { bgzf::Deflater d;
      const int64_t piece[2] = {0, (int64_t)raw.size()};
      bgzf::deflate_pieces(d, raw.data(), piece, 1, 1, packed, nullptr); }
    packed.insert(packed.end(), bgzf::EOF_BLOCK, bgzf::EOF_BLOCK + sizeof bgzf::EOF_BLOCK);
    uint8_t* block = (uint8_t*)malloc(packed.size());
    if (!block) return PLAT_ERR_NOMEM;
    memcpy(block, packed.data(), packed.size());
    *tbi = block; *tbi_len = packed.size();
    if (info) {
        info->lines = W.I.status[tbxindex::ST_LINES]; info->records = W.I.status[tbxindex::ST_RECORDS]; info->runs = W.I.status[tbxindex::ST_RUNS];
        info->contigs = W.I.status[tbxindex::ST_CONTIGS]; info->windows = W.I.status[tbxindex::ST_WINDOWS]; info->seconds = secs(t0, Clock::now());
    }
    return PLAT_OK;
}
