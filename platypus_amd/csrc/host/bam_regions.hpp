// bam_regions.hpp -- plat_call_bam_regions (include/platypus_caller_bam.h): the region loop for raw BAM alignment records.  A second front
// end of fetched_regions.hpp: the records' blobs go to the device as they are, plat_bam_decode_batch (ReadIterator.get,
// htslibWrapper.pyx:328-406, on the device) makes the ASCII tables plat_read_buffers_batch takes, the host reads the decoded per-read arrays,
// CIGAR pairs and bases (no qualities) back for its mirror, and fetchedFinish does the rest.  The host loops over records (their offsets),
// never over bases, qualities or CIGAR words.
// Included at the end of region_caller.cpp, after fetched_regions.hpp.
#pragma once
#include "../../../include/platypus_caller_bam.h"

// referenced weakly, as plat_read_buffers_batch: the CPU suite's stand-in device library predates it
#pragma weak plat_bam_decode_batch

namespace plathost {

// one decode call: the tables' blobs back to back on the device, their records decoded into one table
struct BamDecoded {
    plat_bam_decode_out o;
    int n = 0;
    int64_t status[4] = {0, -1, 0, 0};
    std::vector<int32_t> tableBegin;                                     // [tables + 1] first record of every table
    BamDecoded() { memset(&o, 0, sizeof o); }
};

// the decode of n records of a blob that lies on the device (dOff / dLimit: the records' offsets and limits, on the device)
static void bamDecodeLaunch(Slot& z, FetchedDeviceBuffers& dev, const uint8_t* dBlob, long long bytes, const int64_t* dOff, const int64_t* dLimit, long long n,
                            BamDecoded& d)
{
    d.n = (int)n;
    // every record has 32 fixed bytes and 1.5 bytes per base, 4 per CIGAR operation
    const long long body = std::max(0ll, bytes - 32 * n);
    plat_bam_decode_out& o = d.o;
    o.cap_bases = body * 2 / 3 + n; o.cap_pairs = std::min<long long>(body / 4, INT_MAX);
    o.read_off = dev.alloc<int64_t>((size_t)n + 1); o.cig_off = dev.alloc<int32_t>((size_t)n + 1);
    o.seq = dev.alloc<uint8_t>((size_t)o.cap_bases + PLAT_BLOB_PAD); o.qual = dev.alloc<uint8_t>((size_t)o.cap_bases + PLAT_BLOB_PAD);
    o.cigar = dev.alloc<int16_t>(2 * (size_t)o.cap_pairs + 2);
    o.pos = dev.alloc<int32_t>((size_t)n); o.end = dev.alloc<int32_t>((size_t)n); o.mapq = dev.alloc<uint8_t>((size_t)n);
    o.flags = dev.alloc<int32_t>((size_t)n); o.chrom_id = dev.alloc<int16_t>((size_t)n); o.mate_chrom_id = dev.alloc<int16_t>((size_t)n);
    o.insert_size = dev.alloc<int32_t>((size_t)n); o.mate_pos = dev.alloc<int32_t>((size_t)n);
    o.status = dev.alloc<int64_t>(4);
    ck(plat_bam_decode_batch(z.ctx, d.n, dBlob, bytes, dOff, dLimit, &o, z.stream), "plat_bam_decode_batch");
    ck(plat_memcpy_d2h(z.ctx, d.status, o.status, sizeof d.status, z.stream), "plat_memcpy_d2h");
}

static void bamDecode(Slot& z, FetchedDeviceBuffers& dev, const std::vector<const plat_bam_records*>& tables, BamDecoded& d)
{
    void* st = z.stream;
    long long bytes = 0, n = 0;
    for (const plat_bam_records* t : tables) { bytes += t->n_records ? t->data_len : 0; n += t->n_records; }
    uint8_t* dBlob = dev.alloc<uint8_t>((size_t)bytes);
    std::vector<int64_t> recOff, recLimit;
    recOff.reserve((size_t)n); recLimit.reserve((size_t)n);
    d.tableBegin.push_back(0);
    long long base = 0;
    for (const plat_bam_records* t : tables) {
        if (t->n_records) {
            ck(plat_memcpy_h2d(z.ctx, dBlob + base, t->data, (size_t)t->data_len, st), "plat_memcpy_h2d(records)");
            for (int i = 0; i < t->n_records; ++i) {                       // (an offset outside its own blob stays outside: the device refuses it)
                const int64_t o = t->rec_off[i];
                recOff.push_back(o < 0 || o > t->data_len ? -1 : base + o); recLimit.push_back(base + t->data_len);
            }
            base += t->data_len;
        }
        d.tableBegin.push_back((int32_t)recOff.size());
    }
    const int64_t* dOff = dev.upload(recOff, st);
    const int64_t* dLimit = dev.upload(recLimit, st);
    bamDecodeLaunch(z, dev, dBlob, bytes, dOff, dLimit, n, d);
}

template <class T> static void bamReadBack(Slot& z, std::vector<T>& h, const T* dptr, size_t n) {
    h.resize(n);
    if (n) ck(plat_memcpy_d2h(z.ctx, h.data(), dptr, n * sizeof(T), z.stream), "plat_memcpy_d2h");
}

// the decodes' status blocks, read back: 0, or the error with its message (entry: the entry point's name; stream s = sample s % n_samples of the
// s / n_samples-th loaded region)
static int bamDecodeFailure(plat_caller* c, const std::string& entry, const BamDecoded& F, const BamDecoded& B, const FetchedStage& S,
                            const std::vector<FetchedRegionHead>& heads, int n_regions, int n_samples)
{
    for (const BamDecoded* d : {&F, &B}) {
        if (d->status[0] == 0) continue;
        const long long who = d->status[1];
        const int s = (int)(std::upper_bound(d->tableBegin.begin(), d->tableBegin.end(), (int32_t)who) - d->tableBegin.begin()) - 1;
        int k = 0, left = s / std::max(n_samples, 1);
        for (; k < n_regions; ++k) if (S.loaded[(size_t)k] && left-- == 0) break;
        const std::string what = std::string(d == &F ? "fetched" : "broken-mate") + " record " + std::to_string(who - d->tableBegin[(size_t)s]) + " of " +
                                 fetchedWhere(heads[(size_t)k], k, s % std::max(n_samples, 1));
        if (d->status[0] == PLAT_ERR_OVERFLOW)
            c->lastError = entry + ": the records decode to more bases or CIGAR operations than their bytes can hold (records listed twice or "
                           "overlapping?): first at " + what;
        else
            c->lastError = entry + ": " + what + " cannot be decoded (it runs past its blob, has no bases or no qualities, a CIGAR operation "
                           "above 8, or a length, reference id or position the reference's read would not hold)";
        return (int)d->status[0];
    }
    if (F.status[3] > INT_MAX || B.status[3] > INT_MAX) {
        c->lastError = entry + ": more reads than one call takes (call the region list in parts)";
        return PLAT_ERR_OVERFLOW;
    }
    return PLAT_OK;
}

// What both record front ends leave for fetchedFinish once the decodes have run (and the stream has been waited for): the host mirror read
// back, the fetched table as plat_read_buffers_batch takes it, and every stream's broken mates as a finished table.
static void bamStage(Slot& z, FetchedDeviceBuffers& dev, FetchedStage& S, const BamDecoded& F, const BamDecoded& B, long long nReads, long long nBroken,
                     int nStreams)
{
    // the host mirror: per-read arrays, CIGAR pairs and bases (1 byte per base, no qualities)
    const size_t N = (size_t)nReads, nb = (size_t)F.status[2], np = (size_t)F.status[3];
    bamReadBack(z, S.off, F.o.read_off, N + 1); bamReadBack(z, S.cigOff, F.o.cig_off, N + 1);
    bamReadBack(z, S.pos, F.o.pos, N); bamReadBack(z, S.end, F.o.end, N); bamReadBack(z, S.mapq, F.o.mapq, N);
    bamReadBack(z, S.matePos, F.o.mate_pos, N); bamReadBack(z, S.cigar, F.o.cigar, 2 * np); bamReadBack(z, S.seq, F.o.seq, nb);
    const size_t NB = (size_t)nBroken, bb = (size_t)B.status[2], bp = (size_t)B.status[3];
    std::vector<int64_t> bOff;
    std::vector<int32_t> bCigOff, bPos, bEnd, bFlags, bMatePos;
    std::vector<uint8_t> bMapq, bSeq;
    std::vector<int16_t> bCigar;
    bamReadBack(z, bOff, B.o.read_off, NB + 1); bamReadBack(z, bCigOff, B.o.cig_off, NB + 1); bamReadBack(z, bPos, B.o.pos, NB);
    bamReadBack(z, bEnd, B.o.end, NB); bamReadBack(z, bFlags, B.o.flags, NB); bamReadBack(z, bMatePos, B.o.mate_pos, NB);
    bamReadBack(z, bMapq, B.o.mapq, NB); bamReadBack(z, bCigar, B.o.cigar, 2 * bp); bamReadBack(z, bSeq, B.o.seq, bb);
    ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");
    S.seq.resize(nb + PLAT_BLOB_PAD, 0); S.cigar.push_back(0); S.cigar.push_back(0);
    S.qualBytes = nb + PLAT_BLOB_PAD;
    // the table plat_read_buffers_batch takes: the decode's output as it lies
    std::vector<int32_t> streamOf;
    streamOf.reserve(N);
    for (int s = 0; s < nStreams; ++s) streamOf.insert(streamOf.end(), (size_t)(F.tableBegin[(size_t)s + 1] - F.tableBegin[(size_t)s]), s);
    S.streamBegin = F.tableBegin;
    plat_read_buffers_in& in = S.in;
    in.qc.n_reads = (int)N;
    in.qc.read_qual = F.o.qual; in.qc.read_off = F.o.read_off; in.qc.read_pos = F.o.pos; in.qc.read_mapq = F.o.mapq; in.qc.read_flags = F.o.flags;
    in.qc.chrom_id = F.o.chrom_id; in.qc.mate_chrom_id = F.o.mate_chrom_id; in.qc.insert_size = F.o.insert_size; in.qc.mate_pos = F.o.mate_pos;
    in.qc.cigar = F.o.cigar; in.qc.cig_off = F.o.cig_off; in.qc.stream_of = dev.upload(streamOf, z.stream);
    in.n_streams = nStreams; in.stream_begin = dev.upload(S.streamBegin, z.stream);
    in.read_seq = F.o.seq; in.read_end = F.o.end;
    // broken mates: every stream's table with offsets from 0 (host copies for the host's stages, the decoded arrays on the device)
    std::vector<int64_t> tOff;
    std::vector<int32_t> tCigOff;
    for (int s = 0; s < nStreams; ++s)
        for (int r = B.tableBegin[(size_t)s]; r <= B.tableBegin[(size_t)s + 1]; ++r) {
            tOff.push_back(bOff[(size_t)r] - bOff[(size_t)B.tableBegin[(size_t)s]]);
            tCigOff.push_back(bCigOff[(size_t)r] - bCigOff[(size_t)B.tableBegin[(size_t)s]]);
        }
    const int64_t* dtOff = dev.upload(tOff, z.stream);
    const int32_t* dtCigOff = dev.upload(tCigOff, z.stream);
    S.broken.resize((size_t)nStreams); S.brokenHost.resize((size_t)nStreams);
    for (int s = 0; s < nStreams; ++s) {
        const size_t r0 = (size_t)B.tableBegin[(size_t)s], m = (size_t)B.tableBegin[(size_t)s + 1] - r0, at = r0 + (size_t)s;
        const size_t b0 = (size_t)bOff[r0], b1 = (size_t)bOff[r0 + m], c0 = (size_t)bCigOff[r0], c1 = (size_t)bCigOff[r0 + m];
        FetchedHostTable& h = S.brokenHost[(size_t)s];
        h.off.assign(tOff.begin() + at, tOff.begin() + at + m + 1); h.cigOff.assign(tCigOff.begin() + at, tCigOff.begin() + at + m + 1);
        h.pos.assign(bPos.begin() + r0, bPos.begin() + r0 + m); h.end.assign(bEnd.begin() + r0, bEnd.begin() + r0 + m);
        h.flags.assign(bFlags.begin() + r0, bFlags.begin() + r0 + m); h.matePos.assign(bMatePos.begin() + r0, bMatePos.begin() + r0 + m);
        h.mapq.assign(bMapq.begin() + r0, bMapq.begin() + r0 + m);
        h.seq.assign(bSeq.begin() + b0, bSeq.begin() + b1); h.seq.resize(h.seq.size() + PLAT_BLOB_PAD, 0);
        h.cigar.assign(bCigar.begin() + 2 * c0, bCigar.begin() + 2 * c1); h.cigar.push_back(0); h.cigar.push_back(0);
        plat_read_table& t = S.broken[(size_t)s];
        memset(&t, 0, sizeof t);
        t.n_reads = (int32_t)m; t.encoding = PLAT_READS_ASCII;
        t.seq = h.seq.data(); t.qual = nullptr; t.off = h.off.data(); t.pos = h.pos.data(); t.end = h.end.data(); t.mapq = h.mapq.data();
        t.flags = h.flags.data(); t.mate_pos = h.matePos.data(); t.cigar = h.cigar.data(); t.cig_off = h.cigOff.data();
        if (m) {
            t.dev_seq = B.o.seq + b0; t.dev_qual = B.o.qual + b0; t.dev_off = dtOff + at; t.dev_cig_off = dtCigOff + at;
            t.dev_cigar = B.o.cigar + 2 * c0; t.dev_pos = B.o.pos + r0; t.dev_end = B.o.end + r0; t.dev_mapq = B.o.mapq + r0; t.dev_flags = B.o.flags + r0;
        }
    }
}

}  // namespace plathost

CALLER_EXPORT int plat_call_bam_regions(plat_caller* c, const plat_bam_region* regions, int n_regions, int n_samples,
                                        const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                                        char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats)
{
    SourceLinesGuard sourceGuard(c);
    int rc = checkCallArgs(c, options, out_text, out_len, n_regions, n_samples);
    if (rc != PLAT_OK) return rc;
    if (!qc || (n_regions > 0 && !regions)) return PLAT_ERR_INVALID;
    if (!plat_bam_decode_batch || !plat_read_buffers_batch) {
        c->lastError = "plat_call_bam_regions: the device library has no plat_bam_decode_batch";
        return PLAT_ERR_UNSUPPORTED;
    }
    const auto t0 = Clock::now();
    // loadBAMData's bail-out (:538-541), on record counts, as plat_call_fetched_regions
    const double mr = options->maxReads;
    const long long maxReads = mr >= (double)INT_MAX ? INT_MAX : (mr <= (double)INT_MIN ? INT_MIN : (long long)mr);     // (cdef int maxReads)
    FetchedStage S;
    S.loaded.assign((size_t)n_regions, 0);
    std::vector<FetchedRegionHead> heads;
    std::vector<const plat_bam_records*> fetched, broken;                 // per stream
    long long nReads = 0, nBroken = 0;
    for (int k = 0; k < n_regions; ++k) {
        const plat_bam_region& r = regions[k];
        if (!r.samples) return PLAT_ERR_INVALID;
        heads.push_back(FetchedRegionHead{r.chrom, r.start, r.end, r.contig_seq, r.contig_len, r.dev_contig_seq});
        long long total = 0;
        for (int i = 0; i < n_samples; ++i) {
            for (const plat_bam_records* t : {&r.samples[i].fetched, &r.samples[i].broken_mates})
                if (t->n_records < 0 || (t->n_records && (!t->data || !t->rec_off || t->data_len < 0))) return PLAT_ERR_INVALID;
            total += r.samples[i].fetched.n_records;
        }
        S.loaded[(size_t)k] = !(total > 0 && total >= maxReads);
        if (!S.loaded[(size_t)k]) continue;
        for (int i = 0; i < n_samples; ++i) {
            fetched.push_back(&r.samples[i].fetched); broken.push_back(&r.samples[i].broken_mates);
            nReads += r.samples[i].fetched.n_records; nBroken += r.samples[i].broken_mates.n_records;
            for (const plat_bam_records* t : {&r.samples[i].fetched, &r.samples[i].broken_mates}) S.linkBytes += t->n_records ? t->data_len : 0;
        }
    }
    const int nStreams = (int)fetched.size();
    if (nReads > INT_MAX - 2ll * nStreams - 1 || nBroken > INT_MAX - (long long)nStreams - 1) {
        c->lastError = "plat_call_bam_regions: more reads than one call takes (call the region list in parts)";
        return PLAT_ERR_OVERFLOW;
    }
    S.nStreams = nStreams; S.N = (int)nReads; S.packed = false;
    Slot& z = *c->slots[0];
    FetchedDeviceBuffers dev(z.ctx);
    try {
        BamDecoded F, B;
        bamDecode(z, dev, fetched, F);
        bamDecode(z, dev, broken, B);
        ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");
        rc = bamDecodeFailure(c, "plat_call_bam_regions", F, B, S, heads, n_regions, n_samples);
        if (rc != PLAT_OK) return rc;
        bamStage(z, dev, S, F, B, nReads, nBroken, nStreams);
    } catch (const DeviceError& e) {
        c->lastError = e.what();
        return e.code;
    }
    return fetchedFinish(c, "plat_call_bam_regions", dev, S, heads, n_samples, sample_names, options, qc, out_text, out_len, info, stats, t0);
}
