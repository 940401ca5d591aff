// fetched_regions.hpp -- plat_call_fetched_regions (include/platypus_caller_fetched.h): the region loop for reads as a BAM fetch returns
// them.  In front of the loop: the loader's per-read work of loadBAMData (platypusutils.pyx:505-541) through
// bamReadBuffer.addReadToBuffer (cwindow.pyx:560-595) -- checkAndTrimRead, reads / badReads, isSorted, maxReads -- on the device
// (plat_read_buffers_batch), the buffers gathered there and handed to the loop as device-resident tables (plat_read_table.dev_*).
// PLAT_READS_PACKED fetched tables go through plat_read_buffers_packed_batch instead: QC and trimming on the packed bytes and exceptions,
// no quality array anywhere.
// This file: the tables checked, concatenated and uploaded; the frame of the call and everything from the QC call on are front_end.hpp's.
// Included at the end of region_caller.cpp, after front_end.hpp.
#pragma once

namespace plathost {

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

// The fetched tables of the loaded regions, stream after stream (one stream = one sample of one loaded region), and the broken mates, table
// after table with offsets from 0 per table: concatenated on the host, uploaded once, left in F.S for finish.
static void uploadFetched(FrontCall& F, const plat_fetched_region* regions, long long nBytes, long long nExc)
{
    FetchedStage& S = F.S;
    const std::vector<int>& loaded = S.loaded;
    const int n_regions = F.n_regions, n_samples = F.n_samples, nStreams = S.nStreams;
    const long long nReads = S.N;
    const bool packed = S.packed;
    Slot& z = *F.z;
    FetchedDeviceBuffers& dev = F.dev;
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
    FrontCall F(c, "plat_call_fetched_regions", n_regions, n_samples, sample_names, options, qc, out_text, out_len, info, stats);
    int rc = F.open(regions, true, {(const void*)plat_read_buffers_batch}, "plat_read_buffers_batch");
    if (rc != PLAT_OK) return rc;
    FetchedStage& S = F.S;
    const std::vector<int>& loaded = S.loaded;
    long long nReads = 0, nBytes = 0, nPairs = 0, nBroken = 0, nBrokenPairs = 0, nExc = 0;
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
                if (encoding < 0) { encoding = f.fetched.encoding; firstOfEncoding = F.where(k, i); }
                else if (f.fetched.encoding != encoding) {
                    c->lastError = F.entry + ": the fetched tables of one call share one encoding: the fetched reads of " +
                                   F.where(k, i) + " are " + encodingName(f.fetched.encoding) + ", those of " + firstOfEncoding + " " +
                                   encodingName(encoding);
                    return PLAT_ERR_UNSUPPORTED;
                }
            }
            if (f.fetched.n_reads && (!f.chrom_id || !f.mate_chrom_id || !f.insert_size)) return PLAT_ERR_INVALID;
            total += f.fetched.n_reads;
        }
        S.loaded[(size_t)k] = !F.drops(total);
        if (!loaded[(size_t)k]) continue;
        for (int i = 0; i < n_samples; ++i) {
            const plat_read_table& t = r.samples[i].fetched;
            const plat_read_table& m = r.samples[i].broken_mates;
            nReads += t.n_reads; nBytes += t.n_reads ? t.off[t.n_reads] : 0; nPairs += t.n_reads ? t.cig_off[t.n_reads] : 0;
            nBroken += m.n_reads; nBrokenPairs += m.n_reads ? m.cig_off[m.n_reads] : 0;
            // the bases and qualities that cross the link: 2 bytes per base, or (packed) 1 + 10 per exception (index, base, quality)
            for (const plat_read_table* x : {&t, &m}) {
                const long long nb = x->n_reads ? x->off[x->n_reads] : 0;
                const long long ne = x->n_reads && x->encoding == PLAT_READS_PACKED ? x->n_exceptions : 0;
                S.linkBytes += x->encoding == PLAT_READS_PACKED ? nb + 10 * ne : 2 * nb;
            }
            if (t.n_reads && t.encoding == PLAT_READS_PACKED) nExc += t.n_exceptions;
            ++nStreams;
        }
    }
    const bool packed = S.packed = encoding == PLAT_READS_PACKED;
    if (packed && (rc = F.needs({(const void*)plat_read_buffers_packed_batch}, "plat_read_buffers_packed_batch (PLAT_READS_PACKED fetched tables)")) != PLAT_OK) return rc;
    if ((rc = F.tooMany(nReads, nBroken, nStreams, INT_MAX, std::max(nPairs, nBrokenPairs))) != PLAT_OK) return rc;
    return F.guarded([&] { uploadFetched(F, regions, nBytes, nExc); return F.finish(); });
}
