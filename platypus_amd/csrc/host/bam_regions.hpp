// bam_regions.hpp -- plat_call_bam_regions (include/platypus_caller_bam.h): the region loop for raw BAM alignment records.  A front end on
// front_end.hpp's frame: the records' blobs go to the device as they are (uploadRecords), plat_bam_decode_batch (ReadIterator.get,
// htslibWrapper.pyx:328-406, on the device) makes the ASCII tables plat_read_buffers_batch takes, the host reads the decoded per-read arrays,
// CIGAR pairs and bases (no qualities) back for its mirror, and FrontCall::finish does the rest.  The host loops over records (their
// offsets), never over bases, qualities or CIGAR words.  decodeAndStage is the tail of every front end that holds records (bgzf_regions.hpp,
// rg_regions.hpp).
// Included at the end of region_caller.cpp, after fetched_regions.hpp.
#pragma once
#include "../../../include/platypus_caller_bam.h"
#include "../../../include/platypus_caller_rg.h"                        // (plat_bam_file_records: the uploader takes both tables)

// referenced weakly, as plat_read_buffers_batch: the CPU suite's stand-in device library predates it
#pragma weak plat_bam_decode_batch

namespace plathost {

// a table's own fields (its records are the device's to check)
static bool recordsValid(const plat_bam_records& t) { return t.n_records >= 0 && (!t.n_records || (t.data && t.rec_off && t.data_len >= 0)); }

static const plat_bam_records& recordsOf(const plat_bam_records& t) { return t; }
static const plat_bam_records& recordsOf(const plat_bam_file_records& t) { return t.records; }
static const int32_t* recLenOf(const plat_bam_records&) { return nullptr; }
static const int32_t* recLenOf(const plat_bam_file_records& t) { return t.rec_len; }

// The records of a list of tables (one per stream) on the device: the blobs back to back as they are, and every record's offset and limit
// -- where its rec_len says, or (tables without one) where its blob ends.  Tables with rec_len feed the route, which reads the streams'
// begins on the device.
template <class Table> static RecordList uploadRecords(Slot& z, FetchedDeviceBuffers& dev, const std::vector<const Table*>& tables)
{
    void* st = z.stream;
    RecordList L;
    long long n = 0;
    for (const Table* t : tables) { L.bytes += recordsOf(*t).n_records ? recordsOf(*t).data_len : 0; n += recordsOf(*t).n_records; }
    uint8_t* dBlob = dev.alloc<uint8_t>((size_t)L.bytes);
    std::vector<int64_t> recOff, recLimit;
    recOff.reserve((size_t)n); recLimit.reserve((size_t)n);
    L.begin.assign(1, 0);
    long long base = 0;
    for (const Table* t : tables) {
        const plat_bam_records& r = recordsOf(*t);
        const int32_t* len = recLenOf(*t);
        if (r.n_records) {
            ck(plat_memcpy_h2d(z.ctx, dBlob + base, r.data, (size_t)r.data_len, st), "plat_memcpy_h2d(records)");
            for (int i = 0; i < r.n_records; ++i) {                        // (a record outside its own blob stays outside: the device refuses it)
                const int64_t o = r.rec_off[i], e = len ? o + len[i] : r.data_len;
                const bool in = o >= 0 && o <= r.data_len && e <= r.data_len;
                recOff.push_back(in ? base + o : -1); recLimit.push_back(in || !len ? base + e : -1);
            }
            base += r.data_len;
        }
        L.begin.push_back((int32_t)recOff.size());
    }
    L.blob = dBlob; L.off = dev.upload(recOff, st); L.limit = dev.upload(recLimit, st);
    if (std::is_same<Table, plat_bam_file_records>::value) L.dBegin = dev.upload(L.begin, st);
    return L;
}

// one decode call: the records of a list decoded into one table
struct BamDecoded {
    plat_bam_decode_out o;
    int64_t status[4] = {0, -1, 0, 0};
    BamDecoded() { memset(&o, 0, sizeof o); }
};

// the decode of a list's records enqueued, its status on its way back
static void bamDecodeLaunch(Slot& z, FetchedDeviceBuffers& dev, const RecordList& L, BamDecoded& d)
{
    const long long n = L.n(), bytes = L.bytes;
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
    ck(plat_bam_decode_batch(z.ctx, (int)n, L.blob, bytes, L.off, L.limit, &o, z.stream), "plat_bam_decode_batch");
    ck(plat_memcpy_d2h(z.ctx, d.status, o.status, sizeof d.status, z.stream), "plat_memcpy_d2h");
}

template <class T> static void bamReadBack(Slot& z, std::vector<T>& h, const T* dptr, size_t n) {
    h.resize(n);
    if (n) ck(plat_memcpy_d2h(z.ctx, h.data(), dptr, n * sizeof(T), z.stream), "plat_memcpy_d2h");
}

// the decodes' status blocks, read back: 0, or the error with its message (stream s = sample s % n_samples of the s / n_samples-th loaded
// region)
static int bamDecodeFailure(FrontCall& F, const RecordList& fetched, const BamDecoded& df, const RecordList& broken, const BamDecoded& db)
{
    plat_caller* c = F.c;
    const std::string& entry = F.entry;
    for (const BamDecoded* d : {&df, &db}) {
        if (d->status[0] == 0) continue;
        const std::vector<int32_t>& begin = d == &df ? fetched.begin : broken.begin;
        const long long who = d->status[1];
        const int s = (int)(std::upper_bound(begin.begin(), begin.end(), (int32_t)who) - begin.begin()) - 1;
        const std::string what = std::string(d == &df ? "fetched" : "broken-mate") + " record " + std::to_string(who - begin[(size_t)s]) + " of " +
                                 F.where(F.loadedRegion(s / F.n_samples), s % F.n_samples);
        if (d->status[0] == PLAT_ERR_OVERFLOW)
            c->lastError = entry + ": the records decode to more bases or CIGAR operations than their bytes can hold (records listed twice or "
                           "overlapping?): first at " + what;
        else
            c->lastError = entry + ": " + what + " cannot be decoded (it runs past its blob, has no bases or no qualities, a CIGAR operation "
                           "above 8, or a length, reference id or position the reference's read would not hold)";
        return (int)d->status[0];
    }
    return F.tooMany(F.S.N, 0, F.S.nStreams, INT_MAX, std::max(df.status[3], db.status[3]));     // (the decoded CIGAR pairs are counted in 32 bits too)
}

// What the record front ends leave for finish once the decodes have run (and the stream has been waited for): the host mirror read back,
// the fetched table as plat_read_buffers_batch takes it, and every stream's broken mates as a finished table.
static void bamStage(FrontCall& F, const RecordList& fetched, const BamDecoded& df, const RecordList& broken, const BamDecoded& db)
{
    Slot& z = *F.z;
    FetchedDeviceBuffers& dev = F.dev;
    FetchedStage& S = F.S;
    const int nStreams = S.nStreams;
    const long long nReads = S.N, nBroken = broken.n();
    // the host mirror: per-read arrays, CIGAR pairs and bases (1 byte per base, no qualities)
    const size_t N = (size_t)nReads, nb = (size_t)df.status[2], np = (size_t)df.status[3];
    bamReadBack(z, S.off, df.o.read_off, N + 1); bamReadBack(z, S.cigOff, df.o.cig_off, N + 1);
    bamReadBack(z, S.pos, df.o.pos, N); bamReadBack(z, S.end, df.o.end, N); bamReadBack(z, S.mapq, df.o.mapq, N);
    bamReadBack(z, S.matePos, df.o.mate_pos, N); bamReadBack(z, S.cigar, df.o.cigar, 2 * np); bamReadBack(z, S.seq, df.o.seq, nb);
    const size_t NB = (size_t)nBroken, bb = (size_t)db.status[2], bp = (size_t)db.status[3];
    std::vector<int64_t> bOff;
    std::vector<int32_t> bCigOff, bPos, bEnd, bFlags, bMatePos;
    std::vector<uint8_t> bMapq, bSeq;
    std::vector<int16_t> bCigar;
    bamReadBack(z, bOff, db.o.read_off, NB + 1); bamReadBack(z, bCigOff, db.o.cig_off, NB + 1); bamReadBack(z, bPos, db.o.pos, NB);
    bamReadBack(z, bEnd, db.o.end, NB); bamReadBack(z, bFlags, db.o.flags, NB); bamReadBack(z, bMatePos, db.o.mate_pos, NB);
    bamReadBack(z, bMapq, db.o.mapq, NB); bamReadBack(z, bCigar, db.o.cigar, 2 * bp); bamReadBack(z, bSeq, db.o.seq, bb);
    ck(plat_stream_sync(z.ctx, z.stream), "plat_stream_sync");
    S.seq.resize(nb + PLAT_BLOB_PAD, 0); S.cigar.push_back(0); S.cigar.push_back(0);
    S.qualBytes = nb + PLAT_BLOB_PAD;
    // the table plat_read_buffers_batch takes: the decode's output as it lies
    std::vector<int32_t> streamOf;
    streamOf.reserve(N);
    for (int s = 0; s < nStreams; ++s) streamOf.insert(streamOf.end(), (size_t)(fetched.begin[(size_t)s + 1] - fetched.begin[(size_t)s]), s);
    S.streamBegin = fetched.begin;
    plat_read_buffers_in& in = S.in;
    in.qc.n_reads = (int)N;
    in.qc.read_qual = df.o.qual; in.qc.read_off = df.o.read_off; in.qc.read_pos = df.o.pos; in.qc.read_mapq = df.o.mapq; in.qc.read_flags = df.o.flags;
    in.qc.chrom_id = df.o.chrom_id; in.qc.mate_chrom_id = df.o.mate_chrom_id; in.qc.insert_size = df.o.insert_size; in.qc.mate_pos = df.o.mate_pos;
    in.qc.cigar = df.o.cigar; in.qc.cig_off = df.o.cig_off; in.qc.stream_of = dev.upload(streamOf, z.stream);
    in.n_streams = nStreams; in.stream_begin = dev.upload(S.streamBegin, z.stream);
    in.read_seq = df.o.seq; in.read_end = df.o.end;
    // broken mates: every stream's table with offsets from 0 (host copies for the host's stages, the decoded arrays on the device)
    std::vector<int64_t> tOff;
    std::vector<int32_t> tCigOff;
    for (int s = 0; s < nStreams; ++s)
        for (int r = broken.begin[(size_t)s]; r <= broken.begin[(size_t)s + 1]; ++r) {
            tOff.push_back(bOff[(size_t)r] - bOff[(size_t)broken.begin[(size_t)s]]);
            tCigOff.push_back(bCigOff[(size_t)r] - bCigOff[(size_t)broken.begin[(size_t)s]]);
        }
    const int64_t* dtOff = dev.upload(tOff, z.stream);
    const int32_t* dtCigOff = dev.upload(tCigOff, z.stream);
    S.broken.resize((size_t)nStreams); S.brokenHost.resize((size_t)nStreams);
    for (int s = 0; s < nStreams; ++s) {
        const size_t r0 = (size_t)broken.begin[(size_t)s], m = (size_t)broken.begin[(size_t)s + 1] - r0, at = r0 + (size_t)s;
        const size_t b0 = (size_t)bOff[r0], b1 = (size_t)bOff[r0 + m], c0 = (size_t)bCigOff[r0], c1 = (size_t)bCigOff[r0 + m];
        FetchedHostTable& h = S.brokenHost[(size_t)s];
        h.off.assign(tOff.begin() + at, tOff.begin() + at + m + 1); h.cigOff.assign(tCigOff.begin() + at, tCigOff.begin() + at + m + 1);
        h.pos.assign(bPos.begin() + r0, bPos.begin() + r0 + m); h.end.assign(bEnd.begin() + r0, bEnd.begin() + r0 + m);
        h.flags.assign(bFlags.begin() + r0, bFlags.begin() + r0 + m); h.matePos.assign(bMatePos.begin() + r0, bMatePos.begin() + r0 + m);
        h.mapq.assign(bMapq.begin() + r0, bMapq.begin() + r0 + m);
        h.seq.assign(bSeq.begin() + b0, bSeq.begin() + b1); h.seq.resize(h.seq.size() + PLAT_BLOB_PAD, 0);
        h.cigar.assign(bCigar.begin() + 2 * c0, bCigar.begin() + 2 * c1); h.cigar.push_back(0); h.cigar.push_back(0);
        plat_read_table& t = S.broken[(size_t)s];
        h.pointTo(t, false);
        if (m) {
            t.dev_seq = db.o.seq + b0; t.dev_qual = db.o.qual + b0; t.dev_off = dtOff + at; t.dev_cig_off = dtCigOff + at;
            t.dev_cigar = db.o.cigar + 2 * c0; t.dev_pos = db.o.pos + r0; t.dev_end = db.o.end + r0; t.dev_mapq = db.o.mapq + r0; t.dev_flags = db.o.flags + r0;
        }
    }
}

// The tail of every front end that holds records: each list decoded where it lies (the broken mates' list is made behind the first decode's
// launch, where every one of these calls has put it), one wait, the decodes' refusals, the stage, finish.
template <class MakeBroken> static int decodeAndStage(FrontCall& F, const RecordList& fetched, MakeBroken&& makeBroken)
{
    BamDecoded df, db;
    bamDecodeLaunch(*F.z, F.dev, fetched, df);
    const RecordList broken = makeBroken();
    bamDecodeLaunch(*F.z, F.dev, broken, db);
    ck(plat_stream_sync(F.z->ctx, F.z->stream), "plat_stream_sync");
    const int rc = bamDecodeFailure(F, fetched, df, broken, db);
    if (rc != PLAT_OK) return rc;
    bamStage(F, fetched, df, broken, db);
    return F.finish();
}

}  // namespace plathost

CALLER_EXPORT int plat_call_bam_regions(plat_caller* c, const plat_bam_region* regions, int n_regions, int n_samples,
                                        const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                                        char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats)
{
    FrontCall F(c, "plat_call_bam_regions", n_regions, n_samples, sample_names, options, qc, out_text, out_len, info, stats);
    const int rc = F.open(regions, true, {(const void*)plat_bam_decode_batch, (const void*)plat_read_buffers_batch}, "plat_bam_decode_batch");
    if (rc != PLAT_OK) return rc;
    FetchedStage& S = F.S;
    std::vector<const plat_bam_records*> fetched, broken;                 // per stream
    long long nReads = 0, nBroken = 0;
    for (int k = 0; k < n_regions; ++k) {                                 // (the bail-out on record counts, as plat_call_fetched_regions)
        const plat_bam_region& r = regions[k];
        if (!r.samples) return PLAT_ERR_INVALID;
        long long total = 0;
        for (int i = 0; i < n_samples; ++i) {
            for (const plat_bam_records* t : {&r.samples[i].fetched, &r.samples[i].broken_mates})
                if (!recordsValid(*t)) return PLAT_ERR_INVALID;
            total += r.samples[i].fetched.n_records;
        }
        S.loaded[(size_t)k] = !F.drops(total);
        if (!S.loaded[(size_t)k]) continue;
        for (int i = 0; i < n_samples; ++i) {
            fetched.push_back(&r.samples[i].fetched); broken.push_back(&r.samples[i].broken_mates);
            nReads += r.samples[i].fetched.n_records; nBroken += r.samples[i].broken_mates.n_records;
            for (const plat_bam_records* t : {&r.samples[i].fetched, &r.samples[i].broken_mates}) S.linkBytes += t->n_records ? t->data_len : 0;
        }
    }
    if (F.tooMany(nReads, nBroken, (long long)fetched.size()) != PLAT_OK) return PLAT_ERR_OVERFLOW;
    return F.guarded([&] {
        return decodeAndStage(F, uploadRecords(*F.z, F.dev, fetched), [&] { return uploadRecords(*F.z, F.dev, broken); });
    });
}
