// front_end.hpp -- what the front ends of the region loop share (fetched_regions.hpp, bam_regions.hpp, bgzf_regions.hpp, rg_regions.hpp): the
// frame of one call (FrontCall: the checks at entry, loadBAMData's bail-out, the overflow test, the names of places in messages) and
// everything from the QC call on (FrontCall::finish: checkAndTrimRead, reads / badReads, isSorted on the device --
// plat_read_buffers_batch, plat_read_buffers_packed_batch -- the host's copies of the split tables, the region loop, info and stats).  A
// front end leaves the call's read table on the device plus the host mirror the later stages need (FetchedStage) and ends in finish.
// RecordList is the one form in which raw BAM records reach the decode (bam_regions.hpp), whoever put them on the device.
// Every entry point that runs a batch on slot 0's stream, the side ones too (tabix_source.hpp, index_source.hpp, bgzf_out.hpp, tbi_out.hpp),
// shares the check for device entry points (needsEntryPoints), the one try/catch (guardedEntry) and the call's device memory
// (FetchedDeviceBuffers).
// Included at the end of region_caller.cpp, in front of the four (it calls callRegions and reads plat_caller).
#pragma once
#include <climits>
#include "../../../include/platypus_caller_fetched.h"

// The device entry points are referenced weakly: the CPU test suite links this library against a stand-in device library that predates them
// (the call then returns PLAT_ERR_UNSUPPORTED).
#pragma weak plat_read_buffers_batch
#pragma weak plat_read_buffers_packed_batch

namespace plathost {

// device memory of one call, freed on every way out
struct FetchedDeviceBuffers {
    plat_ctx* ctx = nullptr;
    std::vector<void*> held;
    FetchedDeviceBuffers() {}
    explicit FetchedDeviceBuffers(Slot& z) : ctx(z.ctx) {}
    template <class T> T* alloc(size_t n) {
        void* p = nullptr;
        ck(plat_malloc(ctx, std::max<size_t>(n, 1) * sizeof(T), &p), "plat_malloc");
        held.push_back(p);
        return (T*)p;
    }
    template <class T> T* upload(const std::vector<T>& h, void* stream) {
        T* d = alloc<T>(h.size());
        if (!h.empty()) ck(plat_memcpy_h2d(ctx, d, h.data(), h.size() * sizeof(T), stream), "plat_memcpy_h2d");
        return d;
    }
    // n elements back, behind what the stream holds (the caller waits); a vector: all of it, nothing queued for an empty one
    template <class T> void download(T* host, const T* dev, size_t n, void* stream) { ck(plat_memcpy_d2h(ctx, host, dev, n * sizeof(T), stream), "plat_memcpy_d2h"); }
    template <class T> void download(std::vector<T>& host, const T* dev, void* stream) { if (!host.empty()) download(host.data(), dev, host.size(), stream); }
    ~FetchedDeviceBuffers() { for (void* p : held) plat_free(ctx, p); }
};

// 0, or PLAT_ERR_UNSUPPORTED with its message when one of the device entry points `fns` is not there
inline int needsEntryPoints(plat_caller* c, const std::string& entry, std::initializer_list<const void*> fns, const char* missing) {
    for (const void* f : fns)
        if (!f) { c->lastError = entry + ": the device library has no " + missing; return PLAT_ERR_UNSUPPORTED; }
    return PLAT_OK;
}

// what an exception leaves of a call: a device error's code and text, PLAT_ERR_NOMEM and the entry point's name in front of any other
inline int errorOf(const std::exception& e, const std::string& entry, std::string& text) {
    if (const DeviceError* d = dynamic_cast<const DeviceError*>(&e)) { text = d->what(); return d->code; }
    text = entry + ": " + e.what();
    return PLAT_ERR_NOMEM;
}
// fn() with whatever it throws turned into the call's error: no exception leaves a C entry point
template <class Fn> inline int guardedEntry(plat_caller* c, const std::string& entry, Fn&& fn) {
    try { return fn(); }
    catch (const std::exception& e) { return errorOf(e, entry, c->lastError); }
}

// one buffer (reads or badReads) of one sample as the host's stages see it: per-read arrays and bases, no qualities (packed: the bytes as
// handed over -- the host's stages read their base bits only -- and the exceptions, indexed into the buffer, with the trimmed qualities)
struct FetchedHostTable {
    std::vector<int64_t> off, excIndex;
    std::vector<int32_t> pos, end, flags, matePos, cigOff;
    std::vector<uint8_t> mapq, seq, excBase, excQual;
    std::vector<int16_t> cigar;
    // t: a table of these arrays (its dev_* are the caller's to set)
    void pointTo(plat_read_table& t, bool packed) const {
        memset(&t, 0, sizeof t);
        t.n_reads = (int32_t)pos.size(); t.encoding = packed ? PLAT_READS_PACKED : PLAT_READS_ASCII;
        t.seq = seq.data(); t.qual = nullptr; t.off = off.data(); t.pos = pos.data(); t.end = end.data(); t.mapq = mapq.data();
        t.flags = flags.data(); t.mate_pos = matePos.data(); t.cigar = cigar.data(); t.cig_off = cigOff.data();
        if (packed) {
            t.n_exceptions = (int64_t)excIndex.size();
            t.exc_index = excIndex.data(); t.exc_base = excBase.data(); t.exc_qual = excQual.data();
        }
    }
};

// what the loop needs of a region besides its reads
struct FetchedRegionHead { const char* chrom; int32_t start, end; const uint8_t* contig_seq; int64_t contig_len; const uint8_t* dev_contig_seq; };

// What a front end leaves for finish: the call's fetched table on the device (`in` / `pin`: stream after stream, one stream = one sample of
// one loaded region), the host mirror of its per-read arrays and bases, and every stream's broken mates as a finished table (host arrays
// and dev_*).
struct FetchedStage {
    std::vector<int> loaded;                                             // [n_regions]
    int nStreams = 0, N = 0;
    bool packed = false;
    long long linkBytes = 0;
    std::vector<uint8_t> seq, mapq, excBase, excQual;                    // seq: the bases (packed: the bytes) + PLAT_BLOB_PAD
    std::vector<int64_t> off, excIdx;
    std::vector<int32_t> pos, end, matePos, cigOff, streamBegin;
    std::vector<int16_t> cigar;                                          // + one pair of zeros
    size_t qualBytes = 0;                                                // of in.qc.read_qual, slack included (0: packed)
    plat_read_buffers_in in;
    plat_read_buffers_packed_in pin;
    uint8_t* dExcQual = nullptr;
    std::vector<plat_read_table> broken;                                 // [nStreams]
    std::vector<FetchedHostTable> brokenHost;                            // (front ends that own the broken mates' host arrays)
    FetchedStage() { memset(&in, 0, sizeof in); memset(&pin, 0, sizeof pin); }
};

// Records on the device as the decode takes them: one blob, every record's offset and limit in it (-1: the record leaves its own blob, the
// device refuses it), stream after stream.  The uploader, BgzfStreams::find (bgzf_blocks.hpp) and rgRegroup make one.
struct RecordList {
    const uint8_t* blob = nullptr;
    long long bytes = 0;
    const int64_t* off = nullptr;
    const int64_t* limit = nullptr;
    std::vector<int32_t> begin;                                          // [streams + 1] first record of every stream (host)
    const int32_t* dBegin = nullptr;                                     // the same on the device, where the route reads it
    int nStreams() const { return (int)begin.size() - 1; }
    long long n() const { return begin.empty() ? 0 : begin.back(); }
};

// options.maxReads as the loader holds it (cdef int maxReads)
inline long long maxReadsOf(const plat_caller_options& o) {
    const double mr = o.maxReads;
    return mr >= (double)INT_MAX ? INT_MAX : (mr <= (double)INT_MIN ? INT_MIN : (long long)mr);
}
// loadBAMData's bail-out (platypusutils.pyx:538-541): `totalReads >= maxReads` after each fetched read, summed over the region's
// samples (or files); a region with no reads never gets there
inline bool dropsRegion(long long total, long long maxReads) { return total > 0 && total >= maxReads; }

// One call of a front end: the caller, the entry point's name (for messages), the arguments every front end passes through, slot 0 and
// the call's device memory, the stage it fills and the regions' heads.
struct FrontCall {
    SourceLinesGuard sourceGuard;                                        // (the source lines are gone when the front end returns, however it returns)
    plat_caller* c;
    const std::string entry;
    const int n_regions, n_samples;
    const char* const* sample_names;
    plat_caller_options* options;
    const plat_caller_qc_options* qc;
    char** out_text; size_t* out_len;
    plat_fetched_region_info* info;
    plat_caller_stats* stats;
    Clock::time_point t0;
    long long maxReads = 0;
    Slot* z = nullptr;
    FetchedDeviceBuffers dev;
    FetchedStage S;
    std::vector<FetchedRegionHead> heads;

    FrontCall(plat_caller* c_, const char* entry_, int n_regions_, int n_samples_, const char* const* sample_names_, plat_caller_options* options_,
              const plat_caller_qc_options* qc_, char** out_text_, size_t* out_len_, plat_fetched_region_info* info_, plat_caller_stats* stats_)
        : sourceGuard(c_), c(c_), entry(entry_), n_regions(n_regions_), n_samples(n_samples_), sample_names(sample_names_), options(options_), qc(qc_),
          out_text(out_text_), out_len(out_len_), info(info_), stats(stats_) {}

    int needs(std::initializer_list<const void*> fns, const char* missing) { return needsEntryPoints(c, entry, fns, missing); }

    // The checks at entry, in the order every front end has made them: the call's arguments, the front end's own (argsOk) and the regions
    // pointer, the device entry points; then the clock, maxReads as the loader holds it, slot 0, nothing loaded yet, the regions' heads.
    template <class Region> int open(const Region* regions, bool argsOk, std::initializer_list<const void*> fns, const char* missing) {
        int rc = checkCallArgs(c, options, out_text, out_len, n_regions, n_samples);
        if (rc != PLAT_OK) return rc;
        if (!qc || !argsOk || (n_regions > 0 && !regions)) return PLAT_ERR_INVALID;
        if ((rc = needs(fns, missing)) != PLAT_OK) return rc;
        t0 = Clock::now();
        maxReads = maxReadsOf(*options);
        z = c->slots[0].get();
        dev.ctx = z->ctx;
        S.loaded.assign((size_t)n_regions, 0);
        for (int k = 0; k < n_regions; ++k) {
            const Region& r = regions[k];
            heads.push_back(FetchedRegionHead{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, r.dev_contig_seq});
        }
        return PLAT_OK;
    }

    bool drops(long long total) const { return dropsRegion(total, maxReads); }

    // 0 and the stage's counts set, or PLAT_ERR_OVERFLOW with its message: the reads, broken mates and CIGAR pairs of one call are counted in
    // 32 bits (streamLimit: the read-group calls bound their streams too)
    int tooMany(long long nReads, long long nBroken, long long nStreams, long long streamLimit = INT_MAX, long long nPairs = 0) {
        if (nStreams > streamLimit || nReads > INT_MAX - 2 * nStreams - 1 || nBroken > INT_MAX - nStreams - 1 || nPairs > INT_MAX) {
            c->lastError = entry + ": more reads than one call takes (call the region list in parts)";
            return PLAT_ERR_OVERFLOW;
        }
        S.nStreams = (int)nStreams; S.N = (int)nReads;
        return PLAT_OK;
    }

    template <class Fn> int guarded(Fn&& fn) { return guardedEntry(c, entry, fn); }

    // "region K (chr:a-b), sample I" (unit: what I counts -- a sample, or a file of the merged-file calls)
    std::string where(int k, int i, const char* unit = "sample") const {
        const FetchedRegionHead& r = heads[(size_t)k];
        return "region " + std::to_string(k) + " (" + (r.chrom ? r.chrom : "?") + ":" + std::to_string(r.start) + "-" + std::to_string(r.end) + "), " +
               unit + " " + std::to_string(i);
    }
    // the j-th loaded region's place in the call's list (stream s of n units per region is unit s % n of region loadedRegion(s / n))
    int loadedRegion(int j) const {
        int k = 0;
        for (; k < n_regions; ++k) if (S.loaded[(size_t)k] && j-- == 0) break;
        return k;
    }

    int finish();
};

// Everything from the QC call on: checkAndTrimRead, split and gather on the device, the host's copies of the split tables, the region loop,
// info and stats.
inline int FrontCall::finish()
{
    const int nStreams = S.nStreams, N = S.N;
    const bool packed = S.packed;
    void* st = z->stream;
    plat_readqc_options qo;
    qo.min_good_qual_bases = qc->minGoodQualBases; qo.min_map_qual = qc->minMapQual; qo.min_base_qual = qc->minBaseQual;
    qo.trim_overlapping = qc->trimOverlapping; qo.trim_adapter = qc->trimAdapter; qo.trim_read_flank = qc->trimReadFlank;
    qo.trim_soft_clipped = qc->trimSoftClipped; qo.filter_mate_unmapped = qc->filterReadsWithUnmappedMates;
    qo.filter_mate_distant = qc->filterReadsWithDistantMates; qo.filter_small_insert = qc->filterReadPairsWithSmallInserts;
    qo.filter_duplicates = qc->filterDuplicates;
    plat_read_buffers_tables g;
    g.off = dev.alloc<int64_t>((size_t)N + 2 * (size_t)nStreams); g.cig_off = dev.alloc<int32_t>((size_t)N + 2 * (size_t)nStreams);
    g.seq = dev.alloc<uint8_t>(S.seq.size()); g.qual = packed ? nullptr : dev.alloc<uint8_t>(S.qualBytes); g.cigar = dev.alloc<int16_t>(S.cigar.size());
    g.pos = dev.alloc<int32_t>((size_t)N); g.end = dev.alloc<int32_t>((size_t)N); g.mapq = dev.alloc<uint8_t>((size_t)N);
    g.flags = dev.alloc<int32_t>((size_t)N); g.mate_pos = dev.alloc<int32_t>((size_t)N);
    ck(plat_memset(z->ctx, g.seq, 0, S.seq.size(), st), "plat_memset");       // (the blob's slack: 7-bit bytes for kernels that read whole dwords)
    if (!packed) ck(plat_memset(z->ctx, g.qual, 0, S.qualBytes, st), "plat_memset");
    ck(plat_memset(z->ctx, g.cigar, 0, S.cigar.size() * sizeof(int16_t), st), "plat_memset");
    int32_t* dOk = dev.alloc<int32_t>((size_t)N);
    int32_t* dWhy = dev.alloc<int32_t>((size_t)N);
    int32_t* dPerm = dev.alloc<int32_t>((size_t)N);
    int32_t* dCounts = dev.alloc<int32_t>((size_t)nStreams * 10);
    if (nStreams && packed) ck(plat_read_buffers_packed_batch(z->ctx, &S.pin, &qo, dOk, dWhy, dPerm, dCounts, &g, st), "plat_read_buffers_packed_batch");
    else if (nStreams) ck(plat_read_buffers_batch(z->ctx, &S.in, &qo, dOk, dWhy, dPerm, dCounts, &g, st), "plat_read_buffers_batch");
    // what the host's stages need back: the split, the counts and the flags after QC (QCFail, improper pairs)
    std::vector<int32_t> perm((size_t)N), flagsQc((size_t)N), counts((size_t)nStreams * 10, 0);
    dev.download(perm, dPerm, st); dev.download(flagsQc, S.in.qc.read_flags, st);
    dev.download(counts, dCounts, st);
    if (S.dExcQual) dev.download(S.excQual.data(), S.dExcQual, S.excQual.size(), st);     // (trimmed)
    ck(plat_stream_sync(z->ctx, st), "plat_stream_sync");

    // the buffers, as the host sees them and as the device holds them
    std::vector<std::vector<FetchedHostTable>> host((size_t)nStreams);   // [stream][0 reads, 1 badReads]
    std::vector<plat_sample_reads> sampleReads((size_t)nStreams);
    for (int k = 0, s = 0; k < n_regions; ++k)
    for (int i = 0; i < n_samples && S.loaded[(size_t)k]; ++i, ++s) {    // stream s: sample i of the loaded region k
        const int b = S.streamBegin[(size_t)s], n = S.streamBegin[(size_t)s + 1] - b, nGood = counts[10 * (size_t)s];
        if (nGood < 0 || nGood > n) throw DeviceError(PLAT_ERR_BAD_INPUT, "plat_read_buffers_batch: stream " + std::to_string(s) + " was not split");
        if (counts[10 * (size_t)s + 1]) {
            c->lastError = entry + ": the fetched reads of " + where(k, i) +
                           " are not sorted by position (a BAM fetch is coordinate-sorted; the reference would sort them with an unstable qsort)";
            return PLAT_ERR_BAD_INPUT;
        }
        host[(size_t)s].resize(2);
        int64_t byteAt = S.off[(size_t)b];
        int32_t pairAt = S.cigOff[(size_t)b];
        plat_read_table* tabs[2] = {&sampleReads[(size_t)s].reads, &sampleReads[(size_t)s].bad_reads};
        for (int part = 0; part < 2; ++part) {
            const int p0 = part == 0 ? 0 : nGood, p1 = part == 0 ? nGood : n, m = p1 - p0;
            FetchedHostTable& h = host[(size_t)s][(size_t)part];
            h.off.resize((size_t)m + 1); h.cigOff.resize((size_t)m + 1);
            h.pos.resize((size_t)m); h.end.resize((size_t)m); h.flags.resize((size_t)m); h.matePos.resize((size_t)m); h.mapq.resize((size_t)m);
            int64_t bo = 0;
            int32_t co = 0;
            for (int q = 0; q < m; ++q) {
                const int r = perm[(size_t)(b + p0 + q)];
                h.off[(size_t)q] = bo; h.cigOff[(size_t)q] = co;
                const int64_t len = S.off[(size_t)r + 1] - S.off[(size_t)r];
                const int32_t nc = S.cigOff[(size_t)r + 1] - S.cigOff[(size_t)r];
                h.seq.insert(h.seq.end(), S.seq.begin() + S.off[(size_t)r], S.seq.begin() + S.off[(size_t)r] + len);
                h.cigar.insert(h.cigar.end(), S.cigar.begin() + 2 * (size_t)S.cigOff[(size_t)r], S.cigar.begin() + 2 * ((size_t)S.cigOff[(size_t)r] + (size_t)nc));
                h.pos[(size_t)q] = S.pos[(size_t)r]; h.end[(size_t)q] = S.end[(size_t)r]; h.mapq[(size_t)q] = S.mapq[(size_t)r];
                h.flags[(size_t)q] = flagsQc[(size_t)r]; h.matePos[(size_t)q] = S.matePos[(size_t)r];
                if (!S.excIdx.empty()) {                          // the read's exceptions, re-indexed into this buffer
                    for (auto e = std::lower_bound(S.excIdx.begin(), S.excIdx.end(), S.off[(size_t)r]); e != S.excIdx.end() && *e < S.off[(size_t)r + 1]; ++e) {
                        const size_t x = (size_t)(e - S.excIdx.begin());
                        h.excIndex.push_back(bo + (*e - S.off[(size_t)r])); h.excBase.push_back(S.excBase[x]); h.excQual.push_back(S.excQual[x]);
                    }
                }
                bo += len; co += nc;
            }
            h.off[(size_t)m] = bo; h.cigOff[(size_t)m] = co;
            h.seq.resize(h.seq.size() + PLAT_BLOB_PAD, 0);
            h.cigar.push_back(0); h.cigar.push_back(0);
            plat_read_table& t = *tabs[part];
            h.pointTo(t, packed);
            // the device's copy (plat_read_buffers_batch's layout: `reads` then `badReads` at the stream's input bytes and pairs)
            const size_t oi = (size_t)b + 2 * (size_t)s + (part == 0 ? 0 : (size_t)nGood + 1);
            t.dev_seq = g.seq + byteAt; t.dev_qual = packed ? nullptr : g.qual + byteAt; t.dev_off = g.off + oi; t.dev_cig_off = g.cig_off + oi;
            t.dev_cigar = g.cigar + 2 * (size_t)pairAt; t.dev_pos = g.pos + b + p0; t.dev_end = g.end + b + p0;
            t.dev_mapq = g.mapq + b + p0; t.dev_flags = g.flags + b + p0;
            byteAt += bo; pairAt += co;
        }
        sampleReads[(size_t)s].broken_mates = S.broken[(size_t)s];
    }
    // the loop over the regions that were loaded, with the source lines that came for them
    std::vector<plat_region> called;
    std::vector<plat_source_lines> lines;
    for (int k = 0; k < n_regions; ++k) {
        if (!S.loaded[(size_t)k]) continue;
        const FetchedRegionHead& r = heads[(size_t)k];
        called.push_back(plat_region{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, sampleReads.data() + called.size() * (size_t)n_samples, r.dev_contig_seq});
        if (c->sourceSet) lines.push_back(c->sourceLines[(size_t)k]);
    }
    plat_caller_stats cs;
    const int rc = callRegions(c, called.data(), (int)called.size(), c->sourceSet ? lines.data() : nullptr, n_samples, sample_names, options, out_text, out_len, &cs);
    if (rc != PLAT_OK) return rc;
    std::vector<int64_t> lengths((size_t)n_regions, 0);
    for (int k = 0, j = 0; k < n_regions; ++k) if (S.loaded[(size_t)k]) lengths[(size_t)k] = c->lastLengths[(size_t)j++];
    c->lastLengths.swap(lengths);
    if (info) {
        int s = 0;
        for (int k = 0; k < n_regions; ++k) {
            info[k].loaded = S.loaded[(size_t)k];
            for (int i = 0; i < n_samples; ++i) {
                int32_t* out = info[k].sample_counts ? info[k].sample_counts + 10 * i : nullptr;
                if (!out) continue;
                if (!S.loaded[(size_t)k]) { for (int q = 0; q < 10; ++q) out[q] = 0; continue; }
                const int32_t* sc = counts.data() + 10 * (size_t)(s + i);
                const int n = S.streamBegin[(size_t)(s + i) + 1] - S.streamBegin[(size_t)(s + i)];
                out[0] = sc[0]; out[1] = n - sc[0];
                for (int q = 0; q < 8; ++q) out[2 + q] = sc[2 + q];
            }
            if (S.loaded[(size_t)k]) s += n_samples;
        }
    }
    cs.n_regions = n_regions;
    cs.input_bytes = S.linkBytes;
    cs.seconds_total = secs(t0, Clock::now());
    if (stats) *stats = cs;
    return PLAT_OK;
}

}  // namespace plathost
