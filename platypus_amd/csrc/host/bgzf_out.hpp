// bgzf_out.hpp -- plat_caller_compress_text (include/platypus_caller_bgzfout.h): the record text of a call deflated to BGZF blocks, region by
// region.  The text is cut into slices of whole regions (SLICE_BYTES each, a longer region alone); the workers take slices in turn, each
// on its own context and stream: the slice's bytes and offsets up, plat_bgzf_deflate_batch, status and per-region offsets back, one wait,
// then the compressed bytes alone.  PLAT_CALLER_HOST_DEFLATE=1 runs bgzf::deflate_pieces on the same slices instead.
// Included at the end of region_caller.cpp.
#pragma once
#include "../../../include/platypus_caller_bgzfout.h"
#include "../bgzf_deflate.hpp"

// referenced weakly, as plat_bgzf_inflate_batch (bgzf_blocks.hpp): the CPU suite's stand-in device library predates it
#pragma weak plat_bgzf_deflate_batch

namespace plathost {

struct BgzfOut {
    static constexpr int64_t SLICE_BYTES = (int64_t)32 << 20;
    struct Slice {
        int first = 0, end = 0;                                            // regions [first, end)
        int64_t at = 0, bytes = 0;                                         // its text
        std::vector<uint8_t> data;                                         // its blocks
        std::vector<int64_t> off;                                          // [end - first + 1] into data
    };
    const uint8_t* text;
    const int64_t* regionLen;
    int level;
    std::vector<Slice> slices;

    BgzfOut(const char* text_, const int64_t* region_len, int n_regions, int level_) : text((const uint8_t*)text_), regionLen(region_len), level(level_) {
        int64_t at = 0;
        for (int k = 0; k < n_regions;) {
            Slice s;
            s.first = k; s.at = at;
            do { s.bytes += region_len[k]; ++k; } while (k < n_regions && s.bytes + region_len[k] <= SLICE_BYTES);
            s.end = k;
            at += s.bytes;
            slices.push_back(std::move(s));
        }
    }

    std::vector<int64_t> offsets(const Slice& s) const {
        std::vector<int64_t> off(1, 0);
        for (int k = s.first; k < s.end; ++k) off.push_back(off.back() + regionLen[k]);
        return off;
    }

    void onHost(Slice& s, bgzf::Deflater& d) const {
        const std::vector<int64_t> off = offsets(s);
        s.off.assign(off.size(), 0);
        bgzf::deflate_pieces(d, text + s.at, off.data(), s.end - s.first, level, s.data, s.off.data());
    }

    void onDevice(Slice& s, Slot& z) const {
        FetchedDeviceBuffers dev(z);
        void* st = z.stream;
        const int n = s.end - s.first;
        const std::vector<int64_t> off = offsets(s);
        const int64_t bound = s.bytes + (int64_t)bgzf::BLOCK_OVERHEAD * (s.bytes / (int64_t)bgzf::DEFLATE_PAYLOAD + n);
        uint8_t* dText = dev.alloc<uint8_t>((size_t)s.bytes + PLAT_BLOB_PAD);
        if (s.bytes) ck(plat_memcpy_h2d(z.ctx, dText, text + s.at, (size_t)s.bytes, st), "plat_memcpy_h2d(text)");
        plat_bgzf_deflate_in in;
        memset(&in, 0, sizeof in);
        in.text = dText; in.text_len = s.bytes; in.n_pieces = n; in.level = level; in.piece_off = dev.upload(off, st);
        plat_bgzf_deflate_out o;
        memset(&o, 0, sizeof o);
        o.piece_out_off = dev.alloc<int64_t>((size_t)n + 1); o.status = dev.alloc<int64_t>(4);
        int64_t status[4] = {0, -1, 0, 0};
        s.off.assign((size_t)n + 1, 0);
        // record text deflates to well under half: room for five eighths at first, the size the device names when that is too little
        int64_t cap = std::min(bound, s.bytes / 8 * 5 + 4096);
        for (int attempt = 0;; ++attempt) {
            o.cap_bytes = cap;
            o.data = dev.alloc<uint8_t>((size_t)cap + PLAT_BLOB_PAD);
            ck(plat_bgzf_deflate_batch(z.ctx, &in, &o, st), "plat_bgzf_deflate_batch");
            dev.download(status, o.status, 4, st);
            dev.download(s.off, o.piece_out_off, st);
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
            if (status[0] != PLAT_ERR_OVERFLOW || attempt == 1) break;
            cap = status[2];
        }
        if (status[0] != 0) throw DeviceError((int)status[0], "plat_bgzf_deflate_batch");
        s.data.resize((size_t)status[2]);
        if (!s.data.empty()) {
            ck(plat_memcpy_d2h(z.ctx, s.data.data(), o.data, s.data.size(), st), "plat_memcpy_d2h(blocks)");
            ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");
        }
    }
};

}  // namespace plathost

CALLER_EXPORT int plat_caller_compress_text(plat_caller* c, const char* text, size_t len, const int64_t* region_len, int n_regions, int level, int with_eof,
                                            uint8_t** out, size_t* out_len, int64_t* region_out_len)
{
    if (!c || !out || !out_len || n_regions < 0 || (n_regions > 0 && !region_len) || (len > 0 && !text)) return PLAT_ERR_INVALID;
    *out = nullptr; *out_len = 0;
    if (level < 0 || level > 1) { c->lastError = "plat_caller_compress_text: level " + std::to_string(level) + " (0: stored, 1: deflated)"; return PLAT_ERR_INVALID; }
    { uint64_t sum = 0;
      for (int k = 0; k < n_regions; ++k) {
          if (region_len[k] < 0) { c->lastError = "plat_caller_compress_text: region " + std::to_string(k) + " has a negative length"; return PLAT_ERR_INVALID; }
          sum += (uint64_t)region_len[k];
          if (sum > (uint64_t)len) break;
      }
      if (sum != (uint64_t)len) {
          c->lastError = "plat_caller_compress_text: the regions' lengths do not sum to the text's " + std::to_string(len) + " bytes";
          return PLAT_ERR_INVALID;
      } }
    const bool onHost = Switches::read().hostDeflate;
    const std::string entry = "plat_caller_compress_text";
    const int rc = onHost ? PLAT_OK : needsEntryPoints(c, entry, {(const void*)plat_bgzf_deflate_batch}, "plat_bgzf_deflate_batch");
    if (rc != PLAT_OK) return rc;
    return guardedEntry(c, entry, [&] {
        BgzfOut W(text, region_len, n_regions, level);
        // the workers take slices in turn (an exception cannot cross their threads: each keeps the first error for the call)
        const int nT = (int)std::max<size_t>(1, std::min(c->slots.size(), W.slices.size()));
        std::atomic<size_t> next(0);
        std::mutex errMutex;
        int firstError = PLAT_OK;
        std::string errText;
        auto work = [&](Slot* z) {
            try {
                std::unique_ptr<bgzf::Deflater> d(onHost ? new bgzf::Deflater : nullptr);
                for (size_t k; (k = next.fetch_add(1)) < W.slices.size();) {
                    if (onHost) W.onHost(W.slices[k], *d); else W.onDevice(W.slices[k], *z);
                }
            } catch (const std::exception& e) {
                std::lock_guard<std::mutex> g(errMutex);
                if (firstError == PLAT_OK) firstError = errorOf(e, entry, errText);
                next.store(W.slices.size());
            }
        };
        { std::vector<std::thread> threads;
          for (int i = 1; i < nT; ++i) threads.emplace_back(work, c->slots[(size_t)i].get());
          work(c->slots[0].get());
          for (std::thread& t : threads) t.join(); }
        if (firstError != PLAT_OK) { c->lastError = errText; return firstError; }
        size_t total = with_eof ? sizeof bgzf::EOF_BLOCK : 0;
        for (const BgzfOut::Slice& s : W.slices) total += s.data.size();
        uint8_t* block = (uint8_t*)malloc(total ? total : 1);
        if (!block) return (int)PLAT_ERR_NOMEM;
        size_t at = 0;
        for (const BgzfOut::Slice& s : W.slices) {
            if (!s.data.empty()) memcpy(block + at, s.data.data(), s.data.size());
            if (region_out_len) for (int k = s.first; k < s.end; ++k) region_out_len[k] = s.off[(size_t)(k - s.first) + 1] - s.off[(size_t)(k - s.first)];
            at += s.data.size();
        }
        if (with_eof) memcpy(block + at, bgzf::EOF_BLOCK, sizeof bgzf::EOF_BLOCK);
        *out = block; *out_len = total;
        return (int)PLAT_OK;
    });
}
