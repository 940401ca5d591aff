// fetched_regions.hpp -- plat_call_fetched_regions (include/platypus_caller_fetched.h): the region loop for reads as a BAM fetch returns
// them.  In front of plat_call_regions: the loader's per-read work of loadBAMData (platypusutils.pyx:505-541) through
// bamReadBuffer.addReadToBuffer (cwindow.pyx:560-595) -- checkAndTrimRead, reads / badReads, isSorted, maxReads -- on the device
// (plat_read_buffers_batch), the buffers gathered there and handed to the loop as device-resident tables (plat_read_table.dev_*).
// PLAT_READS_PACKED fetched tables go through plat_read_buffers_packed_batch instead: QC and trimming on the packed bytes and exceptions,
// no quality array anywhere.
// plat_call_bam_regions (include/platypus_caller_bam.h) is a second front end (bam_regions.hpp): both leave the call's read table on the device
// plus the host mirror the later stages need (FetchedStage), and share everything from the QC call on (fetchedFinish).
// Included at the end of region_caller.cpp (it calls plat_call_regions and reads plat_caller).
#pragma once
#include <climits>
#include "../../../include/platypus_caller_fetched.h"

// The device entry point is referenced weakly: the CPU test suite links this library against a stand-in device library that predates it
// (the call then returns PLAT_ERR_UNSUPPORTED).
#pragma weak plat_read_buffers_batch
#pragma weak plat_read_buffers_packed_batch

namespace plathost {

// device memory of one call, freed on every way out
struct FetchedDeviceBuffers {
    plat_ctx* ctx;
    std::vector<void*> held;
    explicit FetchedDeviceBuffers(plat_ctx* c) : ctx(c) {}
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
    ~FetchedDeviceBuffers() { for (void* p : held) plat_free(ctx, p); }
};

// one buffer (reads or badReads) of one sample as the host's stages see it: per-read arrays and bases, no qualities (packed: the bytes as
// handed over -- the host's stages read their base bits only -- and the exceptions, indexed into the buffer, with the trimmed qualities)
struct FetchedHostTable {
    std::vector<int64_t> off, excIndex;
    std::vector<int32_t> pos, end, flags, matePos, cigOff;
    std::vector<uint8_t> mapq, seq, excBase, excQual;
    std::vector<int16_t> cigar;
};

static const char* encodingName(int e) { return e == PLAT_READS_PACKED ? "PLAT_READS_PACKED" : "PLAT_READS_ASCII"; }

// the exceptions of a packed table: ascending indices inside its bytes
static bool exceptionsValid(const plat_read_table& t) {
    if (t.encoding != PLAT_READS_PACKED) return true;
    if (t.n_exceptions < 0) return false;
    if (t.n_exceptions == 0) return true;
    if (!t.exc_index || !t.exc_base || !t.exc_qual) return false;
    const int64_t nb = t.n_reads ? t.off[t.n_reads] : 0;
    for (int64_t e = 0; e < t.n_exceptions; ++e)
        if (t.exc_index[e] < 0 || t.exc_index[e] >= nb || (e && t.exc_index[e] <= t.exc_index[e - 1])) return false;
    return true;
}

// what the loop needs of a region besides its reads
struct FetchedRegionHead { const char* chrom; int32_t start, end; const uint8_t* contig_seq; int64_t contig_len; const uint8_t* dev_contig_seq; };

static std::string fetchedWhere(const FetchedRegionHead& r, int k, int i) {
    return "region " + std::to_string(k) + " (" + (r.chrom ? r.chrom : "?") + ":" + std::to_string(r.start) + "-" + std::to_string(r.end) +
           "), sample " + std::to_string(i);
}
static std::string fetchedWhere(const plat_fetched_region& r, int k, int i) {
    return fetchedWhere(FetchedRegionHead{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, r.dev_contig_seq}, k, i);
}

// What a front end leaves for fetchedFinish: the call's fetched table on the device (`in` / `pin`: stream after stream, one stream = one
// sample of one loaded region), the host mirror of its per-read arrays and bases, and every stream's broken mates as a finished table
// (host arrays and dev_*).
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

// Everything from the QC call on: checkAndTrimRead, split and gather on the device, the host's copies of the split tables, the region loop,
// info and stats.  `who`: the entry point, for messages.
static int fetchedFinish(plat_caller* c, const char* who, FetchedDeviceBuffers& dev, FetchedStage& S, const std::vector<FetchedRegionHead>& regions,
                         int n_samples, const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                         char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats, Clock::time_point t0)
{
    const int n_regions = (int)regions.size(), nStreams = S.nStreams, N = S.N;
    const bool packed = S.packed;
    const std::vector<int>& loaded = S.loaded;
    const std::vector<uint8_t>&seq = S.seq, &mapq = S.mapq, &excBase = S.excBase;
    std::vector<uint8_t>& excQual = S.excQual;
    const std::vector<int64_t>&off = S.off, &excIdx = S.excIdx;
    const std::vector<int32_t>&pos = S.pos, &end = S.end, &matePos = S.matePos, &cigOff = S.cigOff, &streamBegin = S.streamBegin;
    const std::vector<int16_t>& cigar = S.cigar;
    plat_read_buffers_in& in = S.in;
    plat_read_buffers_packed_in& pin = S.pin;
    uint8_t* dExcQual = S.dExcQual;
    Slot& z = *c->slots[0];
    std::vector<std::vector<FetchedHostTable>> host;                     // [stream][0 reads, 1 badReads]
    std::vector<plat_read_table> tabs;                                    // 3 per stream: reads, badReads, brokenMates
    std::vector<plat_sample_reads> sampleReads;
    std::vector<plat_region> called;
    std::vector<int32_t> counts((size_t)nStreams * 10, 0);
    int rc = PLAT_OK;
    try {
        void* st = z.stream;
        int s = 0;
        plat_readqc_options qo;
        qo.min_good_qual_bases = qc->minGoodQualBases; qo.min_map_qual = qc->minMapQual; qo.min_base_qual = qc->minBaseQual;
        qo.trim_overlapping = qc->trimOverlapping; qo.trim_adapter = qc->trimAdapter; qo.trim_read_flank = qc->trimReadFlank;
        qo.trim_soft_clipped = qc->trimSoftClipped; qo.filter_mate_unmapped = qc->filterReadsWithUnmappedMates;
        qo.filter_mate_distant = qc->filterReadsWithDistantMates; qo.filter_small_insert = qc->filterReadPairsWithSmallInserts;
        qo.filter_duplicates = qc->filterDuplicates;
        plat_read_buffers_tables g;
        g.off = dev.alloc<int64_t>((size_t)N + 2 * (size_t)nStreams); g.cig_off = dev.alloc<int32_t>((size_t)N + 2 * (size_t)nStreams);
        g.seq = dev.alloc<uint8_t>(seq.size()); g.qual = packed ? nullptr : dev.alloc<uint8_t>(S.qualBytes); g.cigar = dev.alloc<int16_t>(cigar.size());
        g.pos = dev.alloc<int32_t>((size_t)N); g.end = dev.alloc<int32_t>((size_t)N); g.mapq = dev.alloc<uint8_t>((size_t)N);
        g.flags = dev.alloc<int32_t>((size_t)N); g.mate_pos = dev.alloc<int32_t>((size_t)N);
        ck(plat_memset(z.ctx, g.seq, 0, seq.size(), st), "plat_memset");       // (the blob's slack: 7-bit bytes for kernels that read whole dwords)
        if (!packed) ck(plat_memset(z.ctx, g.qual, 0, S.qualBytes, st), "plat_memset");
        ck(plat_memset(z.ctx, g.cigar, 0, cigar.size() * sizeof(int16_t), st), "plat_memset");
        int32_t* dOk = dev.alloc<int32_t>((size_t)N);
        int32_t* dWhy = dev.alloc<int32_t>((size_t)N);
        int32_t* dPerm = dev.alloc<int32_t>((size_t)N);
        int32_t* dCounts = dev.alloc<int32_t>((size_t)nStreams * 10);
        if (nStreams && packed) ck(plat_read_buffers_packed_batch(z.ctx, &pin, &qo, dOk, dWhy, dPerm, dCounts, &g, st), "plat_read_buffers_packed_batch");
        else if (nStreams) ck(plat_read_buffers_batch(z.ctx, &in, &qo, dOk, dWhy, dPerm, dCounts, &g, st), "plat_read_buffers_batch");
        // what the host's stages need back: the split, the counts and the flags after QC (QCFail, improper pairs)
        std::vector<int32_t> perm((size_t)N), flagsQc((size_t)N);
        if (N) {
            ck(plat_memcpy_d2h(z.ctx, perm.data(), dPerm, sizeof(int32_t) * (size_t)N, st), "plat_memcpy_d2h");
            ck(plat_memcpy_d2h(z.ctx, flagsQc.data(), in.qc.read_flags, sizeof(int32_t) * (size_t)N, st), "plat_memcpy_d2h");
        }
        if (nStreams) ck(plat_memcpy_d2h(z.ctx, counts.data(), dCounts, sizeof(int32_t) * counts.size(), st), "plat_memcpy_d2h");
        if (dExcQual) ck(plat_memcpy_d2h(z.ctx, excQual.data(), dExcQual, excQual.size(), st), "plat_memcpy_d2h");     // (trimmed)
        ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");

        // the buffers, as the host sees them and as the device holds them
        host.resize((size_t)nStreams);
        tabs.resize(3 * (size_t)nStreams);
        s = 0;
        for (int k = 0; k < n_regions; ++k) {
            if (!loaded[(size_t)k]) continue;
            for (int i = 0; i < n_samples; ++i, ++s) {
                const int b = streamBegin[(size_t)s], n = streamBegin[(size_t)s + 1] - b, nGood = counts[10 * (size_t)s];
                if (nGood < 0 || nGood > n) throw DeviceError(PLAT_ERR_BAD_INPUT, "plat_read_buffers_batch: stream " + std::to_string(s) + " was not split");
                if (counts[10 * (size_t)s + 1]) {
                    c->lastError = std::string(who) + ": the fetched reads of " + fetchedWhere(regions[k], k, i) +
                                   " are not sorted by position (a BAM fetch is coordinate-sorted; the reference would sort them with an unstable qsort)";
                    return PLAT_ERR_BAD_INPUT;
                }
                const int64_t byte0 = off[(size_t)b];
                const int32_t pair0 = cigOff[(size_t)b];
                host[(size_t)s].resize(2);
                int64_t byteAt = byte0;
                int32_t pairAt = pair0;
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
                        const int64_t len = off[(size_t)r + 1] - off[(size_t)r];
                        const int32_t nc = cigOff[(size_t)r + 1] - cigOff[(size_t)r];
                        h.seq.insert(h.seq.end(), seq.begin() + off[(size_t)r], seq.begin() + off[(size_t)r] + len);
                        h.cigar.insert(h.cigar.end(), cigar.begin() + 2 * (size_t)cigOff[(size_t)r], cigar.begin() + 2 * ((size_t)cigOff[(size_t)r] + (size_t)nc));
                        h.pos[(size_t)q] = pos[(size_t)r]; h.end[(size_t)q] = end[(size_t)r]; h.mapq[(size_t)q] = mapq[(size_t)r];
                        h.flags[(size_t)q] = flagsQc[(size_t)r]; h.matePos[(size_t)q] = matePos[(size_t)r];
                        if (!excIdx.empty()) {                        // the read's exceptions, re-indexed into this buffer
                            for (auto e = std::lower_bound(excIdx.begin(), excIdx.end(), off[(size_t)r]); e != excIdx.end() && *e < off[(size_t)r + 1]; ++e) {
                                const size_t x = (size_t)(e - excIdx.begin());
                                h.excIndex.push_back(bo + (*e - off[(size_t)r])); h.excBase.push_back(excBase[x]); h.excQual.push_back(excQual[x]);
                            }
                        }
                        bo += len; co += nc;
                    }
                    h.off[(size_t)m] = bo; h.cigOff[(size_t)m] = co;
                    h.seq.resize(h.seq.size() + PLAT_BLOB_PAD, 0);
                    h.cigar.push_back(0); h.cigar.push_back(0);
                    plat_read_table& t = tabs[3 * (size_t)s + (size_t)part];
                    memset(&t, 0, sizeof t);
                    t.n_reads = m; t.encoding = packed ? PLAT_READS_PACKED : PLAT_READS_ASCII;
                    t.seq = h.seq.data(); t.qual = nullptr; t.off = h.off.data(); t.pos = h.pos.data(); t.end = h.end.data(); t.mapq = h.mapq.data();
                    t.flags = h.flags.data(); t.mate_pos = h.matePos.data(); t.cigar = h.cigar.data(); t.cig_off = h.cigOff.data();
                    if (packed) {
                        t.n_exceptions = (int64_t)h.excIndex.size();
                        t.exc_index = h.excIndex.data(); t.exc_base = h.excBase.data(); t.exc_qual = h.excQual.data();
                    }
                    // the device's copy (plat_read_buffers_batch's layout: `reads` then `badReads` at the stream's input bytes and pairs)
                    const size_t oi = (size_t)b + 2 * (size_t)s + (part == 0 ? 0 : (size_t)nGood + 1);
                    t.dev_seq = g.seq + byteAt; t.dev_qual = packed ? nullptr : g.qual + byteAt; t.dev_off = g.off + oi; t.dev_cig_off = g.cig_off + oi;
                    t.dev_cigar = g.cigar + 2 * (size_t)pairAt; t.dev_pos = g.pos + b + p0; t.dev_end = g.end + b + p0;
                    t.dev_mapq = g.mapq + b + p0; t.dev_flags = g.flags + b + p0;
                    byteAt += bo; pairAt += co;
                }
                tabs[3 * (size_t)s + 2] = S.broken[(size_t)s];
            }
        }
    } catch (const DeviceError& e) {
        c->lastError = e.what();
        return e.code;
    }
    // the loop over the regions that were loaded, exactly as plat_call_regions runs it
    sampleReads.resize((size_t)nStreams);
    for (int s = 0; s < nStreams; ++s) sampleReads[(size_t)s] = plat_sample_reads{tabs[3 * (size_t)s], tabs[3 * (size_t)s + 1], tabs[3 * (size_t)s + 2]};
    int s = 0;
    for (int k = 0; k < n_regions; ++k) {
        if (!loaded[(size_t)k]) continue;
        const FetchedRegionHead& r = regions[k];
        called.push_back(plat_region{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, sampleReads.data() + s, r.dev_contig_seq});
        s += n_samples;
    }
    plat_caller_stats st;
    c->keepSourceLines(loaded);                                          // (plat_caller_set_source_lines lists every region of the front end's call)
    rc = plat_call_regions(c, called.data(), (int)called.size(), n_samples, sample_names, options, out_text, out_len, &st);
    if (rc != PLAT_OK) return rc;
    std::vector<int64_t> lengths((size_t)n_regions, 0);
    for (int k = 0, j = 0; k < n_regions; ++k) if (loaded[(size_t)k]) lengths[(size_t)k] = c->lastLengths[(size_t)j++];
    c->lastLengths.swap(lengths);
    if (info) {
        s = 0;
        for (int k = 0; k < n_regions; ++k) {
            info[k].loaded = loaded[(size_t)k];
            for (int i = 0; i < n_samples; ++i) {
                int32_t* out = info[k].sample_counts ? info[k].sample_counts + 10 * i : nullptr;
                if (!out) continue;
                if (!loaded[(size_t)k]) { for (int q = 0; q < 10; ++q) out[q] = 0; continue; }
                const int32_t* cs = counts.data() + 10 * (size_t)(s + i);
                const int n = streamBegin[(size_t)(s + i) + 1] - streamBegin[(size_t)(s + i)];
                out[0] = cs[0]; out[1] = n - cs[0];
                for (int q = 0; q < 8; ++q) out[2 + q] = cs[2 + q];
            }
            if (loaded[(size_t)k]) s += n_samples;
        }
    }
    st.n_regions = n_regions;
    st.input_bytes = S.linkBytes;
    st.seconds_total = secs(t0, Clock::now());
    if (stats) *stats = st;
    return PLAT_OK;
}

}  // namespace plathost

CALLER_EXPORT void plat_caller_default_qc_options(plat_caller_qc_options* o) {
    if (!o) return;
    o->minGoodQualBases = 20; o->minMapQual = 20; o->minBaseQual = 20;
    o->trimOverlapping = 1; o->trimAdapter = 1; o->trimReadFlank = 0; o->trimSoftClipped = 1;
    o->filterDuplicates = 1; o->filterReadsWithUnmappedMates = 1; o->filterReadsWithDistantMates = 1; o->filterReadPairsWithSmallInserts = 1;
}

CALLER_EXPORT int plat_call_fetched_regions(plat_caller* c, const plat_fetched_region* regions, int n_regions, int n_samples,
                                            const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                                            char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats)
{
    SourceLinesGuard sourceGuard(c);
    int rc = checkCallArgs(c, options, out_text, out_len, n_regions, n_samples);
    if (rc != PLAT_OK) return rc;
    if (!qc || (n_regions > 0 && !regions)) return PLAT_ERR_INVALID;
    if (!plat_read_buffers_batch) {
        c->lastError = "plat_call_fetched_regions: the device library has no plat_read_buffers_batch";
        return PLAT_ERR_UNSUPPORTED;
    }
    const auto t0 = Clock::now();
    // loadBAMData's bail-out (:538-541): `totalReads >= maxReads` after each fetched read, summed over the samples; a region with no reads
    // never gets there
    const double mr = options->maxReads;
    const long long maxReads = mr >= (double)INT_MAX ? INT_MAX : (mr <= (double)INT_MIN ? INT_MIN : (long long)mr);     // (cdef int maxReads)
    std::vector<int> loaded((size_t)n_regions, 0);
    long long nReads = 0, nBytes = 0, nPairs = 0, nBroken = 0, nBrokenBytes = 0, nBrokenPairs = 0, nExc = 0, linkBytes = 0;
    int nStreams = 0;
    int encoding = -1;                                                   // of the call's fetched tables (one for all)
    std::string firstOfEncoding;
    for (int k = 0; k < n_regions; ++k) {
        const plat_fetched_region& r = regions[k];
        if (!r.samples) return PLAT_ERR_INVALID;
        long long total = 0;
        for (int i = 0; i < n_samples; ++i) {
            const plat_read_table* tabs[2] = {&r.samples[i].fetched, &r.samples[i].broken_mates};
            for (const plat_read_table* t : tabs) {
                if (t->n_reads < 0) return PLAT_ERR_INVALID;
                if (t->encoding != PLAT_READS_ASCII && t->encoding != PLAT_READS_PACKED) return PLAT_ERR_INVALID;
                if (t->n_reads && (!t->seq || (t->encoding == PLAT_READS_ASCII && !t->qual) || !t->off || !t->pos || !t->end || !t->mapq ||
                                   !t->flags || !t->mate_pos || !t->cig_off || (t->cig_off[t->n_reads] && !t->cigar) || t->off[0] != 0 || t->cig_off[0] != 0))
                    return PLAT_ERR_INVALID;
                if (!exceptionsValid(*t)) return PLAT_ERR_INVALID;
            }
            const plat_fetched_reads& f = r.samples[i];
            if (f.fetched.n_reads) {                                     // (an empty table has no bytes to encode)
                if (encoding < 0) { encoding = f.fetched.encoding; firstOfEncoding = fetchedWhere(r, k, i); }
                else if (f.fetched.encoding != encoding) {
                    c->lastError = std::string("plat_call_fetched_regions: the fetched tables of one call share one encoding: the fetched reads of ") +
                                   fetchedWhere(r, k, i) + " are " + encodingName(f.fetched.encoding) + ", those of " + firstOfEncoding + " " +
                                   encodingName(encoding);
                    return PLAT_ERR_UNSUPPORTED;
                }
            }
            if (f.fetched.n_reads && (!f.chrom_id || !f.mate_chrom_id || !f.insert_size)) return PLAT_ERR_INVALID;
            total += f.fetched.n_reads;
        }
        loaded[(size_t)k] = !(total > 0 && total >= maxReads);
        if (!loaded[(size_t)k]) continue;
        for (int i = 0; i < n_samples; ++i) {
            const plat_read_table& t = r.samples[i].fetched;
            const plat_read_table& m = r.samples[i].broken_mates;
            nReads += t.n_reads; nBytes += t.n_reads ? t.off[t.n_reads] : 0; nPairs += t.n_reads ? t.cig_off[t.n_reads] : 0;
            nBroken += m.n_reads; nBrokenBytes += m.n_reads ? m.off[m.n_reads] : 0; nBrokenPairs += m.n_reads ? m.cig_off[m.n_reads] : 0;
            // the bases and qualities that cross the link: 2 bytes per base, or (packed) 1 + 10 per exception (index, base, quality)
            for (const plat_read_table* x : {&t, &m}) {
                const long long nb = x->n_reads ? x->off[x->n_reads] : 0;
                const long long ne = x->n_reads && x->encoding == PLAT_READS_PACKED ? x->n_exceptions : 0;
                linkBytes += x->encoding == PLAT_READS_PACKED ? nb + 10 * ne : 2 * nb;
            }
            if (t.n_reads && t.encoding == PLAT_READS_PACKED) nExc += t.n_exceptions;
            ++nStreams;
        }
    }
    const bool packed = encoding == PLAT_READS_PACKED;
    if (packed && !plat_read_buffers_packed_batch) {
        c->lastError = "plat_call_fetched_regions: the device library has no plat_read_buffers_packed_batch (PLAT_READS_PACKED fetched tables)";
        return PLAT_ERR_UNSUPPORTED;
    }
    if (nReads > INT_MAX - 2ll * nStreams - 1 || nBroken > INT_MAX - (long long)nStreams - 1 || nPairs > INT_MAX || nBrokenPairs > INT_MAX) {
        c->lastError = "plat_call_fetched_regions: more reads than one call takes (call the region list in parts)";
        return PLAT_ERR_OVERFLOW;
    }
    Slot& z = *c->slots[0];
    FetchedDeviceBuffers dev(z.ctx);
    FetchedStage S;
    S.loaded = loaded; S.nStreams = nStreams; S.N = (int)nReads; S.linkBytes = linkBytes; S.packed = packed;
    std::vector<FetchedRegionHead> heads;
    for (int k = 0; k < n_regions; ++k)
        heads.push_back(FetchedRegionHead{regions[k].chrom, regions[k].start, regions[k].end, regions[k].contig_seq, regions[k].contig_len, regions[k].dev_contig_seq});
    try {
        // the fetched tables, stream after stream (one stream = one sample of one loaded region), and the broken mates, table after table
        // with offsets from 0 per table
        std::vector<uint8_t>&seq = S.seq, &mapq = S.mapq, &excBase = S.excBase, &excQual = S.excQual;
        std::vector<uint8_t> qual, bSeq, bQual, bMapq;
        std::vector<int64_t>&off = S.off, &excIdx = S.excIdx;
        std::vector<int64_t> bOff;
        std::vector<int32_t>&pos = S.pos, &end = S.end, &matePos = S.matePos, &cigOff = S.cigOff, &streamBegin = S.streamBegin;
        std::vector<int32_t> flags, insert, streamOf, bPos, bEnd, bFlags, bCigOff;
        std::vector<int16_t>& cigar = S.cigar;
        std::vector<int16_t> chrom, mateChrom, bCigar;
        std::vector<long long> bOffAt, bByteAt, bQualAt, bPairAt, bReadAt;
        seq.reserve((size_t)nBytes + PLAT_BLOB_PAD);
        if (!packed) qual.reserve((size_t)nBytes + PLAT_BLOB_PAD);
        excIdx.reserve((size_t)nExc); excBase.reserve((size_t)nExc); excQual.reserve((size_t)nExc);
        off.reserve((size_t)nReads + 1); cigOff.reserve((size_t)nReads + 1);
        streamBegin.push_back(0);
        int s = 0;
        for (int k = 0; k < n_regions; ++k) {
            if (!loaded[(size_t)k]) continue;
            for (int i = 0; i < n_samples; ++i, ++s) {
                const plat_fetched_reads& f = regions[k].samples[i];
                const plat_read_table& t = f.fetched;
                const int n = t.n_reads;
                const int64_t b0 = (int64_t)seq.size();
                const int32_t c0 = (int32_t)cigar.size() / 2;
                if (n) {
                    const size_t nb = (size_t)t.off[n], nc = (size_t)t.cig_off[n];
                    seq.insert(seq.end(), t.seq, t.seq + nb);
                    if (!packed) qual.insert(qual.end(), t.qual, t.qual + nb);
                    for (int64_t e = 0; packed && e < t.n_exceptions; ++e) {       // (ascending: each table's lie above the tables' before)
                        excIdx.push_back(b0 + t.exc_index[e]); excBase.push_back(t.exc_base[e]); excQual.push_back(t.exc_qual[e]);
                    }
                    for (int r = 0; r < n; ++r) { off.push_back(b0 + t.off[r]); cigOff.push_back(c0 + t.cig_off[r]); }
                    pos.insert(pos.end(), t.pos, t.pos + n); end.insert(end.end(), t.end, t.end + n); mapq.insert(mapq.end(), t.mapq, t.mapq + n);
                    flags.insert(flags.end(), t.flags, t.flags + n); matePos.insert(matePos.end(), t.mate_pos, t.mate_pos + n);
                    chrom.insert(chrom.end(), f.chrom_id, f.chrom_id + n); mateChrom.insert(mateChrom.end(), f.mate_chrom_id, f.mate_chrom_id + n);
                    insert.insert(insert.end(), f.insert_size, f.insert_size + n);
                    if (nc) cigar.insert(cigar.end(), t.cigar, t.cigar + 2 * nc);
                    streamOf.insert(streamOf.end(), (size_t)n, s);
                }
                streamBegin.push_back((int32_t)pos.size());
                const plat_read_table& m = f.broken_mates;
                bOffAt.push_back((long long)bOff.size()); bByteAt.push_back((long long)bSeq.size()); bPairAt.push_back((long long)bCigar.size() / 2);
                bReadAt.push_back((long long)bPos.size()); bQualAt.push_back((long long)bQual.size());
                if (m.n_reads) {                                      // (a packed table: its bytes only; its exceptions stay in the caller's arrays)
                    const size_t nb = (size_t)m.off[m.n_reads], nc = (size_t)m.cig_off[m.n_reads];
                    bSeq.insert(bSeq.end(), m.seq, m.seq + nb);
                    if (m.encoding == PLAT_READS_ASCII) bQual.insert(bQual.end(), m.qual, m.qual + nb);
                    bOff.insert(bOff.end(), m.off, m.off + m.n_reads + 1); bCigOff.insert(bCigOff.end(), m.cig_off, m.cig_off + m.n_reads + 1);
                    bPos.insert(bPos.end(), m.pos, m.pos + m.n_reads); bEnd.insert(bEnd.end(), m.end, m.end + m.n_reads);
                    bMapq.insert(bMapq.end(), m.mapq, m.mapq + m.n_reads); bFlags.insert(bFlags.end(), m.flags, m.flags + m.n_reads);
                    if (nc) bCigar.insert(bCigar.end(), m.cigar, m.cigar + 2 * nc);
                }
            }
        }
        off.push_back((int64_t)seq.size()); cigOff.push_back((int32_t)cigar.size() / 2);
        cigar.push_back(0); cigar.push_back(0); bCigar.push_back(0); bCigar.push_back(0);
        seq.resize(seq.size() + PLAT_BLOB_PAD, 0);
        if (!packed) qual.resize(qual.size() + PLAT_BLOB_PAD, 0);
        bSeq.resize(bSeq.size() + PLAT_BLOB_PAD, 0); bQual.resize(bQual.size() + PLAT_BLOB_PAD, 0);
        const int N = (int)nReads;

        // upload once; QC, split and gather on the device
        void* st = z.stream;
        plat_read_buffers_in& in = S.in;
        in.qc.n_reads = N;
        in.qc.read_qual = packed ? nullptr : dev.upload(qual, st); in.qc.read_off = dev.upload(off, st); in.qc.read_pos = dev.upload(pos, st);
        in.qc.read_mapq = dev.upload(mapq, st); in.qc.read_flags = dev.upload(flags, st); in.qc.chrom_id = dev.upload(chrom, st);
        in.qc.mate_chrom_id = dev.upload(mateChrom, st); in.qc.insert_size = dev.upload(insert, st); in.qc.mate_pos = dev.upload(matePos, st);
        in.qc.cigar = dev.upload(cigar, st); in.qc.cig_off = dev.upload(cigOff, st); in.qc.stream_of = dev.upload(streamOf, st);
        in.n_streams = nStreams; in.stream_begin = dev.upload(streamBegin, st);
        in.read_seq = dev.upload(seq, st); in.read_end = dev.upload(end, st);
        plat_read_buffers_packed_in& pin = S.pin;
        S.qualBytes = qual.size();
        uint8_t*& dExcQual = S.dExcQual;
        if (packed) {
            pin.qc = in.qc; pin.n_streams = in.n_streams; pin.stream_begin = in.stream_begin;
            pin.read_packed = const_cast<uint8_t*>(in.read_seq); pin.read_end = in.read_end;
            pin.n_exc = (int64_t)excIdx.size();
            if (!excIdx.empty()) { pin.exc_index = dev.upload(excIdx, st); dExcQual = dev.upload(excQual, st); pin.exc_qual = dExcQual; }
        }
        // broken mates: as handed over, resident
        uint8_t* dbSeq = dev.upload(bSeq, st); uint8_t* dbQual = dev.upload(bQual, st); int64_t* dbOff = dev.upload(bOff, st);
        int32_t* dbPos = dev.upload(bPos, st); int32_t* dbEnd = dev.upload(bEnd, st); uint8_t* dbMapq = dev.upload(bMapq, st);
        int32_t* dbFlags = dev.upload(bFlags, st); int16_t* dbCigar = dev.upload(bCigar, st); int32_t* dbCigOff = dev.upload(bCigOff, st);
        S.broken.resize((size_t)nStreams);
        s = 0;
        for (int k = 0; k < n_regions; ++k) {
            if (!loaded[(size_t)k]) continue;
            for (int i = 0; i < n_samples; ++i, ++s) {
                const plat_read_table& m = regions[k].samples[i].broken_mates;
                plat_read_table& t = S.broken[(size_t)s];
                t = m;
                t.dev_seq = dbSeq + bByteAt[(size_t)s]; t.dev_qual = m.encoding == PLAT_READS_ASCII ? dbQual + bQualAt[(size_t)s] : nullptr;
                t.dev_off = dbOff + bOffAt[(size_t)s];
                t.dev_cig_off = dbCigOff + bOffAt[(size_t)s]; t.dev_cigar = dbCigar + 2 * bPairAt[(size_t)s];
                const long long r0 = bReadAt[(size_t)s];
                t.dev_pos = dbPos + r0; t.dev_end = dbEnd + r0; t.dev_mapq = dbMapq + r0; t.dev_flags = dbFlags + r0;
                if (!m.n_reads) { t.dev_off = nullptr; t.dev_seq = nullptr; t.dev_qual = nullptr; }
            }
        }
    } catch (const DeviceError& e) {
        c->lastError = e.what();
        return e.code;
    }
    return fetchedFinish(c, "plat_call_fetched_regions", dev, S, heads, n_samples, sample_names, options, qc, out_text, out_len, info, stats, t0);
}
