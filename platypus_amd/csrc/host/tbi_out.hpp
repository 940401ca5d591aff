// tbi_out.hpp -- plat_caller_index_bgzf (include/platypus_caller_tbi.h): the tabix index of a whole .vcf.gz.  The file is one chunk of a
// block list (bgzf_blocks.hpp: the walk over the block headers, an empty block with data behind it refused; the file goes up in one
// copy), plat_bgzf_inflate_batch and plat_tabix_index_batch run back to back on slot 0's stream, one wait for their status blocks, then
// runs, names and windows come back and tbxindex::finish (csrc/tabix_index.hpp) makes the index of them, deflated by
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
    plat_bgzf_chunk file;
    const std::string entry = "plat_caller_index_bgzf";
    BgzfBlockList L;                                                      // the file's blocks up to the last that holds data
    std::vector<int64_t> blkAddr;                                         // their addresses in the file, and the address behind them
    int64_t allBlocks = 0;
    tbxindex::Intermediate I;
    std::vector<std::string> names;
    int deviceCalls = 0;

    TbiOut(plat_caller* c_, const uint8_t* file_, size_t len) : c(c_), L(entry, [](const BgzfChunkAt&) { return std::string(); }, true, c_->lastError) {
        memset(&file, 0, sizeof file);
        file.data = file_; file.data_len = (int64_t)len; file.end_coffset = -1;
    }

    // the chain walked; the empty blocks at the file's end (the EOF block) are no work for the inflate and no address of a line
    int walk() {
        const int rc = L.add(0, 0, 0, file);
        if (rc != PLAT_OK) return rc;
        allBlocks = L.nBlocks();
        size_t nData = L.blkOff.size();
        while (nData > 0 && L.inflatedEnd((int)nData - 1) == L.blkInflated[nData - 1]) --nData;
        blkAddr.assign(L.blkOff.begin(), L.blkOff.begin() + (long)nData);
        blkAddr.push_back(nData < L.blkOff.size() ? L.blkOff[nData] : file.data_len);
        L.blkOff.resize(nData); L.blkLimit.resize(nData); L.blkInflated.resize(nData);
        L.chunkAt[0].blkEnd = (int)nData;
        return PLAT_OK;
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
        FetchedDeviceBuffers dev(z);
        void* st = z.stream;
        const int nBlocks = L.nBlocks();
        const int64_t inflated = L.inflated;
        const plat_bgzf_inflate_out io = L.inflateOnDevice(z, dev, false, "plat_memcpy_h2d(file)");      // (no limits: one chunk, the blob's end is its end)
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
            if (attempt == 0) dev.download(inflateStatus, io.status, 4, st);
            dev.download(I.status, o.status, (size_t)tbxindex::ST_WORDS, st);
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
            if (inflateStatus[0] != 0) return L.blockRefused(inflateStatus[1], PLAT_ERR_BAD_INPUT);
            if (I.status[tbxindex::ST_VERDICT] != PLAT_ERR_OVERFLOW || attempt == 1) break;
            capRuns = I.status[tbxindex::ST_RUNS]; capWindows = I.status[tbxindex::ST_WINDOWS]; capNameBytes = I.status[tbxindex::ST_NAME_BYTES];
        }
        if (I.status[tbxindex::ST_VERDICT] != 0) return verdict();
        const size_t nRuns = (size_t)I.status[tbxindex::ST_RUNS], nRef = (size_t)I.status[tbxindex::ST_CONTIGS], nWin = (size_t)I.status[tbxindex::ST_WINDOWS];
        I.runTid.resize(nRuns); I.runBin.resize(nRuns); I.runU.resize(nRuns); I.nameOff.resize(nRef); I.nameLen.resize(nRef); I.linFirst.resize(nRef + 1); I.lin.resize(nWin);
        dev.download(I.runTid, o.run_tid, st); dev.download(I.runBin, o.run_bin, st); dev.download(I.runU, o.run_u, st);
        dev.download(I.nameOff, o.name_off, st); dev.download(I.nameLen, o.name_len, st);
        dev.download(I.linFirst, o.lin_first, st); dev.download(I.lin, o.lin, st);
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
        std::vector<uint8_t> data;
        const int64_t bad = L.inflateOnHost(data, PLAT_BLOB_PAD);
        if (bad >= 0) return L.blockRefused(bad, PLAT_ERR_BAD_INPUT);
        std::vector<int64_t> outOff = L.blkInflated;
        outOff.push_back(L.inflated);
        tbxindex::build_serial(data.data(), L.inflated, outOff.data(), blkAddr.data(), L.nBlocks(), I);
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
    const std::string entry = "plat_caller_index_bgzf";
    int rc = onHost ? PLAT_OK : needsEntryPoints(c, entry, {(const void*)plat_bgzf_inflate_batch, (const void*)plat_tabix_index_batch}, "plat_tabix_index_batch");
    if (rc != PLAT_OK) return rc;
    return guardedEntry(c, entry, [&] {
        TbiOut W(c, file, len);
        int rc = W.walk();
        if (rc != PLAT_OK) return rc;
        rc = onHost ? W.onHost() : W.onDevice();
        if (info) {
            info->n_blocks = W.allBlocks; info->compressed_bytes = (int64_t)len; info->inflated_bytes = W.L.inflated; info->device_calls = W.deviceCalls;
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
        if (!block) return (int)PLAT_ERR_NOMEM;
        memcpy(block, packed.data(), packed.size());
        *tbi = block; *tbi_len = packed.size();
        if (info) {
            info->lines = W.I.status[tbxindex::ST_LINES]; info->records = W.I.status[tbxindex::ST_RECORDS]; info->runs = W.I.status[tbxindex::ST_RUNS];
            info->contigs = W.I.status[tbxindex::ST_CONTIGS]; info->windows = W.I.status[tbxindex::ST_WINDOWS]; info->seconds = secs(t0, Clock::now());
        }
        return (int)PLAT_OK;
    });
}
