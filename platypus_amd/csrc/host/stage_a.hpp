// stage_a.hpp -- A: the chunk's read table, the candidate scan (+ merge, + stage B on the device launched behind it), the assembler tiles
// (native region loop, libplat_caller.so: see region_caller.cpp for the stage map and the reference citations)
#pragma once
#include "chunk.hpp"

// The entry points that read packed bases where they lie are referenced weakly, as plat_read_buffers_batch: the CPU suite's stand-in device
// library predates them.  A device library without ALL of them: every chunk is expanded as before.
#pragma weak plat_concat_read_tables_src
#pragma weak plat_pack_codes_pieces
#pragma weak plat_candidates_batch_packed
#pragma weak plat_gather_reads_packed
#pragma weak plat_variant_read_stats_packed_batch

namespace plathost {

struct TableSurvey {                                                        // what one walk over the chunk's tables finds
    size_t nReads[3] = {0, 0, 0}, N = 0, B = 0, Cg = 0, nExc = 0;          // reads (per kind: reads, badReads, brokenMates; in all), bytes of bases, CIGAR pairs, exceptions
    bool anyPacked = false, allPacked = true, excRegular = true;           // (excRegular: no exception with a byte other than A, C, G, T, N)
    bool cols = true;                                                       // every table has its per-read arrays on the device already (plat_concat_read_tables)
};
// ... and what filling the table leaves for the first pass: the pieces of packed bytes to expand (in t_pieces), their exceptions; bytes that crossed the link
struct FilledTable { int nPieces = 0; size_t mostPiece = 0, nExc = 0, inBytes = 0; };

static TableSurvey surveyTables(const std::vector<RegionWork*>& regions) {
    TableSurvey v;
    for (RegionWork* r : regions)
        for (SampleView& sv : r->samples) {
            const TableView* tv[3] = {&sv.reads, &sv.bad, &sv.broken};
            for (int k = 0; k < 3; ++k) {
                const plat_read_table& t = *tv[k]->t;
                v.nReads[k] += (size_t)t.n_reads; v.N += (size_t)t.n_reads; v.B += (size_t)t.off[t.n_reads]; v.Cg += (size_t)t.cig_off[t.n_reads];
                if (t.encoding == PLAT_READS_PACKED) {
                    v.anyPacked = true; v.nExc += (size_t)std::max<int64_t>(t.n_exceptions, 0);
                    for (int64_t e = 0; e < t.n_exceptions && v.excRegular; ++e) v.excRegular = memchr("ACGTN", t.exc_base[e], 5) != nullptr;
                }
                else if (t.encoding != PLAT_READS_ASCII) throw DeviceError(PLAT_ERR_INVALID, "plat_read_table.encoding");
                else if (t.n_reads) v.allPacked = false;
                if (t.n_reads && !(t.dev_off && t.dev_pos && t.dev_end && t.dev_mapq && t.dev_flags && t.dev_cigar && t.dev_cig_off && t.dev_seq)) v.cols = false;
            }
        }
    if (v.N > 0x7FFFFFF0ull) throw DeviceError(PLAT_ERR_OVERFLOW, "chunk read table");
    return v;
}

// Every read out of a packed table and no exception with a byte other than A, C, G, T, N (the promise the scan on codes asks for): the first pass writes
// the bases' 2-bit codes next to the expanded bytes (Codes) -- or the codes ALONE (Packed): the chunk is not expanded at all; the scan, the read statistics
// and the gathers take a read's letters and qualities from its packed bytes where they lie (t_src); t_seq keeps its place but holds only the read-side alleles
// the scan leaves at its records' offsets, and there is no t_qual.  PLAT_CALLER_EXPAND or a device library without the entry points: Codes (which firstPass()
// takes back to Bytes when the device library has no scan on codes either); PLAT_CALLER_NO_CODES: Bytes.
static ReadPath planReadPath(const TableSurvey& v, const Switches& sw) {
    if (!(v.anyPacked && v.allPacked && v.excRegular && v.B > 0) || sw.noCodes) return ReadPath::Bytes;
    const bool haveDirect = plat_concat_read_tables_src && plat_pack_codes_pieces && plat_candidates_batch_packed && plat_gather_reads_packed &&
                            plat_variant_read_stats_packed_batch;
    return haveDirect && !sw.expand ? ReadPath::Packed : ReadPath::Codes;
}

// one table's entry of plat_concat_read_tables[_src]: its per-read arrays on the device and where it goes in the chunk table
template <class D> static D& describeTable(D& d, const plat_read_table& t, int scan, size_t ri, size_t bo, size_t co) {
    d.off = t.dev_off; d.pos = t.dev_pos; d.end = t.dev_end; d.mapq = t.dev_mapq; d.flags = t.dev_flags; d.cigar = t.dev_cigar; d.cig_off = t.dev_cig_off;
    d.n = t.n_reads; d.scan = scan; d.first_read = (int64_t)ri; d.first_byte = (int64_t)bo; d.first_pair = (int64_t)co;
    return d;
}

// (tables lie back to back in the chunk blob: read i's bytes are [t_off[i], t_off[i + 1]) for every consumer.  A packed table that is
//  resident on the device is expanded straight from there; plat_unpack_reads reads a source of another misalignment with unaligned loads)
inline FilledTable Chunk::fillTable(const TableSurvey& v) {
    Slot& z = s;
    const bool direct = z.path == ReadPath::Packed, cols = v.cols;
    const size_t N = v.N, B = v.B, Cg = v.Cg;
    z.t_seq.reserve(z.ctx, B + PLAT_BLOB_PAD, false, true, z.stream);
    if (!direct) z.t_qual.reserve(z.ctx, B + PLAT_BLOB_PAD, false, true, z.stream);
    if (v.anyPacked) z.t_pack.reserve(z.ctx, B + PLAT_BLOB_PAD, false, true, z.stream);
    Layout L;
    L.add(z.t_excidx, v.nExc + 1); L.add(z.t_excb, v.nExc + 1); L.add(z.t_excq, v.nExc + 1);
    L.add(z.t_off, N + 1); L.add(z.t_pos, N + 1); L.add(z.t_end, N + 1); L.add(z.t_flags, N + 1); L.add(z.t_mapq, N + 1); L.add(z.t_cigoff, N + 1);
    L.add(z.t_cigar, 2 * Cg + 2); L.add(z.t_region, v.nReads[0] + 1);
    if (direct) L.add(z.t_src, N + 1);
    L.commit(z, z.a_tab);
    Layout LD;
    size_t nDesc = 0;
    int mostPerTable = 0;                                               // (tables described to plat_concat_read_tables; most reads in one)
    const size_t nTables = 3 * regions.size() * (regions.empty() ? 0 : regions[0]->samples.size());
    LD.add(z.t_pieces, nTables + 1);
    if (cols && direct) LD.add(z.t_sdesc, nTables + 1);
    else if (cols) LD.add(z.t_desc, nTables + 1);
    LD.commit(z, z.a_desc);
    FilledTable f;
    plat_unpack_piece* pieces = z.t_pieces.h;
    bool lastInPack = false;                                            // the last piece lies in t_pack (not in a caller's resident table)
    size_t ri = 0, bo = 0, co = 0;
    for (int k = 0; k < 3; ++k) {
        int scan = 0;                                                   // (the (region, sample) pair: the scan id of its `reads`)
        for (RegionWork* r : regions)
            for (SampleView& sv : r->samples) {
                TableView& tv = k == 0 ? sv.reads : (k == 1 ? sv.bad : sv.broken);
                const plat_read_table& t = *tv.t;
                const int n = t.n_reads;
                tv.base = (int64_t)ri; tv.blobBase = (int64_t)bo;
                maxReadLen = std::max(maxReadLen, tv.maxLen);
                const size_t nb = (size_t)t.off[n], nc = (size_t)t.cig_off[n];
                // (a packed table's bytes on the device: resident, or its place in t_pack)
                const uint8_t* tabSrc = t.dev_seq ? t.dev_seq : z.t_pack.d + bo;
                if (nb && t.encoding == PLAT_READS_PACKED) {            // one byte per base crosses the link (or none: dev_seq); expanded by firstPass()
                    if (!t.dev_seq) ck(plat_memcpy_h2d(z.ctx, z.t_pack.d + bo, t.seq, nb, z.stream), "plat_memcpy_h2d(packed)");
                    const size_t ne = (size_t)std::max<int64_t>(t.n_exceptions, 0);
                    for (size_t e = 0; e < ne; ++e) {                   // (exceptions are indexed from the chunk blob's first byte)
                        z.t_excidx.h[f.nExc + e] = t.exc_index[e] + (int64_t)bo; z.t_excb.h[f.nExc + e] = t.exc_base[e]; z.t_excq.h[f.nExc + e] = t.exc_qual[e];
                    }
                    // every packed table of the chunk is expanded by ONE launch (plat_unpack_reads_pieces): tables that follow each other in t_pack join into one piece
                    plat_unpack_piece* last = f.nPieces ? &pieces[f.nPieces - 1] : nullptr;
                    if (!t.dev_seq && lastInPack && last->dst + last->n == (int64_t)bo) last->n += (int64_t)nb;
                    else { last = &pieces[f.nPieces++]; *last = plat_unpack_piece{tabSrc, (int64_t)bo, (int64_t)nb}; }
                    lastInPack = !t.dev_seq;
                    f.mostPiece = std::max(f.mostPiece, (size_t)last->n); tabPackedBytes += (int64_t)nb;
                    f.nExc += ne; f.inBytes += (t.dev_seq ? 0 : nb) + 10 * ne;
                } else if (nb && t.dev_seq && t.dev_qual) {            // resident in HBM already
                    ck(plat_memcpy_d2d(z.ctx, z.t_seq.d + bo, t.dev_seq, nb, z.stream), "plat_memcpy_d2d(seq)");
                    ck(plat_memcpy_d2d(z.ctx, z.t_qual.d + bo, t.dev_qual, nb, z.stream), "plat_memcpy_d2d(qual)");
                } else if (nb) {                                       // bases and qualities go straight from the caller's memory
                    ck(plat_memcpy_h2d(z.ctx, z.t_seq.d + bo, t.seq, nb, z.stream), "plat_memcpy_h2d(seq)");
                    ck(plat_memcpy_h2d(z.ctx, z.t_qual.d + bo, t.qual, nb, z.stream), "plat_memcpy_h2d(qual)");
                    f.inBytes += 2 * nb;
                }
                if (cols && n) {
                    if (direct) describeTable(z.t_sdesc.h[nDesc++], t, k == 0 ? scan : -1, ri, bo, co).src = tabSrc;
                    else describeTable(z.t_desc.h[nDesc++], t, k == 0 ? scan : -1, ri, bo, co);
                    mostPerTable = std::max(mostPerTable, n);
                } else if (!cols) {
                    for (int i = 0; i < n; ++i) {
                        z.t_off.h[ri + i] = (int64_t)bo + t.off[i];
                        z.t_cigoff.h[ri + i] = (int32_t)(co + (size_t)t.cig_off[i]);
                        if (direct) z.t_src.h[ri + i] = tabSrc + t.off[i];
                    }
                    if (n) {
                        memcpy(z.t_pos.h + ri, t.pos, sizeof(int32_t) * (size_t)n); memcpy(z.t_end.h + ri, t.end, sizeof(int32_t) * (size_t)n);
                        memcpy(z.t_flags.h + ri, t.flags, sizeof(int32_t) * (size_t)n); memcpy(z.t_mapq.h + ri, t.mapq, (size_t)n);
                        if (nc) memcpy(z.t_cigar.h + 2 * co, t.cigar, sizeof(int16_t) * 2 * nc);
                        if (k == 0) for (int i = 0; i < n; ++i) z.t_region.h[ri + i] = scan;
                    }
                }
                ri += (size_t)n; bo += nb; co += nc;
                ++scan;
            }
        nScan = scan;
    }
    if (cols) {
        L.uploadFirst(z, z.a_tab, 3);                                   // (the exceptions of packed tables; the per-read arrays are made on the device)
        if (nDesc) LD.upload(z, z.a_desc);
        if (nDesc && direct)
            ck(plat_concat_read_tables_src(z.ctx, (int)nDesc, mostPerTable, z.t_sdesc.d, z.t_off.d, z.t_pos.d, z.t_end.d, z.t_mapq.d, z.t_flags.d, z.t_cigoff.d, z.t_cigar.d,
                                           z.t_region.d, z.t_src.d, (int64_t)N, (int64_t)B, (int64_t)Cg, z.stream), "plat_concat_read_tables_src");
        else if (nDesc)
            ck(plat_concat_read_tables(z.ctx, (int)nDesc, mostPerTable, z.t_desc.d, z.t_off.d, z.t_pos.d, z.t_end.d, z.t_mapq.d, z.t_flags.d, z.t_cigoff.d, z.t_cigar.d,
                                       z.t_region.d, (int64_t)N, (int64_t)B, (int64_t)Cg, z.stream), "plat_concat_read_tables");
    }
    if (!cols || !nDesc) {
        z.t_off.h[N] = (int64_t)B; z.t_cigoff.h[N] = (int32_t)Cg;
        z.t_cigar.h[2 * Cg] = 0; z.t_cigar.h[2 * Cg + 1] = 0;
        L.upload(z, z.a_tab);
    }
    return f;
}

// the first pass over the packed bytes: ONE launch for every piece -- the codes alone (Packed), bytes + codes (Codes), or the bytes (Bytes)
inline void Chunk::firstPass(const TableSurvey& v, const FilledTable& f) {
    if (!f.nPieces) return;
    Slot& z = s;
    const int64_t B = (int64_t)v.B, nE = (int64_t)f.nExc, most = (int64_t)f.mostPiece;
    ck(plat_memcpy_h2d(z.ctx, z.t_pieces.d, z.t_pieces.h, (size_t)f.nPieces * sizeof(plat_unpack_piece), z.stream), "plat_memcpy_h2d(pieces)");
    if (z.path != ReadPath::Bytes) z.t_codes.reserve(z.ctx, ((size_t)B + 15) / 16 + 16, false);
    if (z.path == ReadPath::Packed)                                     // the codes alone: the bytes stay where they are
        ck(plat_pack_codes_pieces(z.ctx, f.nPieces, most, z.t_pieces.d, z.t_codes.d, B, nE, z.t_excidx.d, z.t_excb.d, z.stream), "plat_pack_codes_pieces");
    else if (z.path == ReadPath::Codes) {
        const int rcu = plat_unpack_reads_pieces_codes(z.ctx, f.nPieces, most, z.t_pieces.d, z.t_seq.d, z.t_qual.d, z.t_codes.d, B, nE, z.t_excidx.d, z.t_excb.d,
                                                       z.t_excq.d, z.stream);
        if (rcu == PLAT_ERR_UNSUPPORTED) z.path = ReadPath::Bytes;      // a device library without the entry point: the chunk ends on the byte path
        else ck(rcu, "plat_unpack_reads_pieces_codes");
    }
    z.pk = plat_packed_reads{z.path == ReadPath::Packed ? z.t_src.d : nullptr, nE, z.t_excidx.d, z.t_excb.d, z.t_excq.d};
    if (z.path == ReadPath::Bytes)
        ck(plat_unpack_reads_pieces(z.ctx, f.nPieces, most, z.t_pieces.d, z.t_seq.d, z.t_qual.d, B, nE, z.t_excidx.d, z.t_excb.d, z.t_excq.d, z.stream),
           "plat_unpack_reads_pieces");
}

// -- A: one device table for every read of the chunk; layout: all `reads` of every (region, sample), then all badReads, then all brokenMates
inline void Chunk::uploadReads() {
    const TableSurvey v = surveyTables(regions);
    s.path = planReadPath(v, o.sw);
    const FilledTable f = fillTable(v);
    firstPass(v, f);
    tabBlobBytes = (int64_t)v.B;
    nGood = v.nReads[0]; nBad = v.nReads[1]; nBroken = v.nReads[2];
    std::lock_guard<std::mutex> g(stMutex);
    st.n_reads += (int64_t)v.N;
    st.input_bytes += (int64_t)f.inBytes;
}

// -- A2: VariantCandidateGenerator.addCandidatesFromReads over the `reads` of every (region, sample) (variant.pyx:459-751)
inline void Chunk::scanCandidates() {
    Slot& z = s;
    std::vector<int64_t> refoff{0};
    std::vector<int32_t> rss, clen, scanbegin, scanlongest;
    // every region with its contig on the device already: the reference windows are put together there (plat_copy_pieces)
    bool refResident = !regions.empty();
    for (RegionWork* r : regions) refResident = refResident && r->in->dev_contig_seq != nullptr;
    std::vector<plat_unpack_piece> pieces;
    size_t blobLen = 0, mostRef = 0;
    for (RegionWork* r : regions)
        for (size_t i = 0; i < r->samples.size(); ++i) {
            scanbegin.push_back((int32_t)r->samples[i].reads.base); scanlongest.push_back(r->samples[i].reads.longest);
            const int64_t a = std::max<int64_t>(0, (int64_t)r->in->start - 2000);                   // variant.pyx:486-488
            const int64_t e = std::min<int64_t>((int64_t)r->in->end + 2000, r->fa.len - 1);
            if (e < a) throw WindowError("Cannot have beginPos > endPos in getSequence");
            if (refResident) pieces.push_back(plat_unpack_piece{r->in->dev_contig_seq + a, (int64_t)blobLen, e - a});
            blobLen += (size_t)(e - a); mostRef = std::max(mostRef, (size_t)(e - a));
            refoff.push_back((int64_t)blobLen);
            rss.push_back((int32_t)a); clen.push_back((int32_t)r->fa.len);
        }
    {
        Layout L;
        scanbegin.push_back((int32_t)nGood);
        L.put(z.c_refoff, refoff); L.put(z.c_rss, rss); L.put(z.c_clen, clen); L.put(z.c_scanbegin, scanbegin); L.put(z.c_scanlongest, scanlongest);
        if (refResident) L.add(z.c_pieces, pieces.size() + 1); else L.add(z.c_ref, blobLen + PLAT_BLOB_PAD);
        L.commit(z, z.a_cin);
        if (refResident) {
            for (size_t q = 0; q < pieces.size(); ++q) z.c_pieces.h[q] = pieces[q];
            z.c_refdev.reserve(z.ctx, blobLen + PLAT_BLOB_PAD, false, true, z.stream);
            refDev = z.c_refdev.d;
        } else {
            size_t at = 0;
            for (RegionWork* r : regions)
                for (size_t i = 0; i < r->samples.size(); ++i) {
                    const int64_t a = std::max<int64_t>(0, (int64_t)r->in->start - 2000), e = std::min<int64_t>((int64_t)r->in->end + 2000, r->fa.len - 1);
                    memcpy(z.c_ref.h + at, r->fa.seq + a, (size_t)(e - a));
                    at += (size_t)(e - a);
                }
            memset(z.c_ref.h + blobLen, 0, PLAT_BLOB_PAD);
            refDev = z.c_ref.d;
        }
        L.upload(z, z.a_cin);
        if (refResident) ck(plat_copy_pieces(z.ctx, (int)pieces.size(), (int64_t)mostRef, z.c_pieces.d, z.c_refdev.d, z.stream), "plat_copy_pieces");
    }
    refBlob.clear();                                                    // (the host's copy of the windows is made when a host stage asks for it: hostRefBlob)
    if (nGood == 0) { hostTally = true; deviceB = false; return; }      // nothing to scan: the (empty) host tally
    plat_candidate_batch cb;
    memset(&cb, 0, sizeof cb);
    cb.n_regions = nScan; cb.n_reads = (int32_t)nGood;
    cb.ref_seq = refDev; cb.ref_off = z.c_refoff.d; cb.ref_seq_start = z.c_rss.d; cb.contig_len = z.c_clen.d;
    cb.read_seq = z.t_seq.d; cb.read_qual = z.t_qual.d; cb.read_off = z.t_off.d; cb.read_pos = z.t_pos.d; cb.read_flags = z.t_flags.d;
    cb.cigar = z.t_cigar.d; cb.cig_off = z.t_cigoff.d;
    hostTally = o.sw.hostTally;                                         // (measurements / tests: merge the records on the host)
    for (;;) {
        // records stay on the device when the merge kernel can take them: c_cnt / c_status / c_rec are laid out for a download
        // all the same (the host tally needs them when a scan overflows the kernel's table)
        Layout LO;
        LO.add(z.c_cnt, nGood); LO.add(z.c_status, nGood); LO.add(z.c_rec, nGood * (size_t)maxPerRead * 5);
        LO.commit(z, z.a_cout);
        recArenaBytes = LO.total; recordsOnHost = false;
        int rcs = PLAT_ERR_UNSUPPORTED;                                 // (PLAT_OK: a scan on codes has run)
        if (z.path != ReadPath::Bytes) {                                // the scan on 2-bit codes: the reference blob's codes first (a few MB per chunk)
            z.c_refcodes.reserve(z.ctx, (blobLen + 15) / 16 + 16, false); z.c_refirr.reserve(z.ctx, (size_t)nScan + 1, false);
            rcs = plat_ref_codes(z.ctx, nScan, refDev, z.c_refoff.d, (int64_t)blobLen, z.c_refcodes.d, z.c_refirr.d, z.stream);
        }
        switch (z.path) {
        case ReadPath::Packed:                                          // letters and qualities from the packed bytes; leaves its records' alleles in t_seq
            ck(rcs, "plat_ref_codes");                                  // (no expanded bytes to fall back to)
            cb.read_qual = nullptr;
            ck(plat_candidates_batch_packed(z.ctx, &cb, &z.pk, z.t_codes.d, z.c_refcodes.d, z.c_refirr.d, o.minFlank, o.minBaseQual, o.genSNPs, o.genIndels, maxPerRead,
                                            z.t_region.d, z.c_rec.d, z.c_cnt.d, z.c_status.d, z.stream), "plat_candidates_batch_packed");
            break;
        case ReadPath::Codes:                                           // (a device library without either entry point: the byte scan below)
            if (rcs == PLAT_OK)
                rcs = plat_candidates_batch_codes(z.ctx, &cb, z.t_codes.d, z.c_refcodes.d, z.c_refirr.d, o.minFlank, o.minBaseQual, o.genSNPs, o.genIndels, maxPerRead,
                                                  z.t_region.d, z.c_rec.d, z.c_cnt.d, z.c_status.d, z.stream);
            if (rcs != PLAT_ERR_UNSUPPORTED) ck(rcs, "plat_candidates_batch_codes");
            break;
        case ReadPath::Bytes: break;
        }
        if (rcs != PLAT_OK)                                             // the byte scan
            ck(plat_candidates_batch(z.ctx, &cb, o.minFlank, o.minBaseQual, o.genSNPs, o.genIndels, maxPerRead, z.t_region.d, z.c_rec.d, z.c_cnt.d,
                                     z.c_status.d, z.stream), "plat_candidates_batch");
        int need = 0;
        if (!hostTally) {
            // addVariantToList + the per-sample support filter on the device (variant.pyx:499-527, variantcaller.pyx:456-467)
            Layout LM;
            LM.add(z.m_n, (size_t)nScan * 2); LM.add(z.m_cand, (size_t)nScan * mergeCap * 8);
            LM.commit(z, z.a_mout);
            {
                // (its table is 64 KB per scan in the context's scratch: a cohort too wide for it falls back to the host tally, it does not fail the call)
                const int rcm = plat_candidates_merge_batch(z.ctx, &cb, z.t_end.d, nScan, z.c_scanbegin.d, z.c_scanlongest.d, maxPerRead, z.c_rec.d, z.c_cnt.d,
                                                            z.c_status.d, o.minVarFreq, mergeCap, z.m_cand.d, z.m_n.d, z.stream);
                // (no room for the table: the records this scan has just written are merged on the host instead -- they are NOT scanned again;
                //  a device that is really out of memory fails the next allocation of the chunk with the same code, loudly)
                if (rcm == PLAT_ERR_NOMEM) hostTally = true;
                else ck(rcm, "plat_candidates_merge_batch");
            }
            if (!hostTally) {
                lmLayout = LM;
                if (deviceB) launchStageB();
                // (host stage B may have to replay a region's dictionaries from the scan's records: a chunk of small regions brings them
                //  along now -- one copy behind the merge's -- instead of two copies and a wait per region that needs them later)
                const bool recordsAlong = !deviceB && LO.total <= ((size_t)4 << 20);
                if (deviceB) LM.downloadFirst(z, z.a_mout, 1);                              // (only the counts: the candidates stay on the device)
                else { LM.download(z, z.a_mout); if (recordsAlong) LO.download(z, z.a_cout); }
                z.sync("candidate scan");
                for (int g = 0; g < nScan; ++g) {
                    const int st_ = z.m_n.h[2 * g + 1];
                    if (st_ == PLAT_ERR_BAD_INPUT) throw DeviceError(PLAT_ERR_BAD_INPUT, "a read reaches outside the reference window handed over, or read pointers out of order");
                    if (st_ <= -(1 << 20)) need = std::max(need, -st_ - (1 << 20));
                    else if (st_ != 0) hostTally = true;                // more distinct records / candidates than the kernel takes
                }
                if (!need && !hostTally) { recordsOnHost = recordsAlong; break; }
                if (need) { maxPerRead = need; continue; }
            }
        }
        LO.download(z, z.a_cout);
        z.sync("candidate scan");
        recordsOnHost = true;
        for (size_t i = 0; i < nGood; ++i) {
            if (z.c_status.h[i] == PLAT_ERR_BAD_INPUT) throw DeviceError(PLAT_ERR_BAD_INPUT, "a read reaches outside the reference window handed over");
            if (z.c_status.h[i] == PLAT_ERR_OVERFLOW) need = std::max(need, z.c_cnt.h[i]);
        }
        if (!need) break;
        maxPerRead = need;                                              // a read with more candidates than its slice: again with room for it
    }
    if (hostTally) deviceB = false;
}

// assemble=1: the tiles of every region of the chunk in ONE assembler launch (variantcaller.pyx:496-519).  Two halves: assembleLaunch() puts the
// batch together, sizes it itself (plat_assemble_batch_async: no read-back, no wait) and leaves launch + download on the stream BEFORE the
// candidate scan's work, so that the scan's one wait covers the assembler too; assembleCollect() turns the tuples into Variants.
inline void Chunk::assembleLaunch() {
    asmN = 0;
    if (!o.assemble) return;
    Slot& z = s;
    const auto t0 = Clock::now();
    const int size = o.assemblyRegionSize;
    if (size <= 0) throw DeviceError(PLAT_ERR_INVALID, "assemblyRegionSize");
    const int shift = std::max(100, std::min(1000, size / 2));
    std::vector<Tile>& tiles = asmTiles;
    tiles.clear();
    std::vector<int64_t> refoff{0}, roff{0};
    std::vector<int32_t> refstart, astart, aend, rbegin{0}, src;
    std::string blob;
    for (RegionWork* rp : regions) {
        RegionWork& r = *rp;
        r.cur.assign(r.samples.size(), Ptrs{0, 0, 0, 0, 0, 0});
        for (int64_t a0 = r.in->start; a0 < r.in->end; a0 += shift) {
            const int assemStart = (int)a0, assemEnd = (int)std::min<int64_t>(a0 + size, r.in->end);
            const int refStart = std::max(0, assemStart - size);
            const std::string refSeq = r.fa.getSequence(refStart, (int64_t)assemEnd + size);
            // doWeNeedToAssembleThisRegion: the window pointers move to the tile whatever the answer
            bool need = o.assembleAll != 0;
            for (size_t i = 0; i < r.samples.size(); ++i) {
                Ptrs& p = r.cur[i];
                r.samples[i].reads.overlapRange(assemStart, assemEnd, p.gs, p.ge);
                r.samples[i].bad.overlapRange(assemStart, assemEnd, p.bs, p.be);
                r.samples[i].broken.matePosRange(assemStart, assemEnd, p.ks, p.ke);
            }
            for (size_t i = 0; !need && i < r.samples.size(); ++i) {
                const Ptrs& p = r.cur[i];
                const double n = p.ge - p.gs, nBad = p.be - p.bs;
                if (n == 0) continue;
                double gaps = 0, improper = 0;                           // countAlignmentGaps / countImproperPairs (cwindow.pyx:598-647): reads + badReads
                auto scan = [&](const TableView& tv, int b, int e) {
                    for (int q = b; q < e; ++q) {
                        for (int c = tv.t->cig_off[q]; c < tv.t->cig_off[q + 1]; ++c) { const int op = tv.t->cigar[2 * c]; gaps += op >= 1 && op <= 4; }
                        improper += !(tv.t->flags[q] & 2);
                    }
                };
                scan(r.samples[i].reads, p.gs, p.ge); scan(r.samples[i].bad, p.bs, p.be);
                if (gaps / n > 2 || improper / (n + nBad) > 0.1) need = true;
            }
            if (!need) continue;
            tiles.push_back(Tile{regionSlot(r.index), assemStart, assemEnd, refStart});
            blob += refSeq;
            refoff.push_back((int64_t)blob.size());
            refstart.push_back(refStart); astart.push_back(assemStart); aend.push_back(assemEnd);
            for (size_t i = 0; i < r.samples.size(); ++i) {
                const Ptrs& p = r.cur[i];
                auto take = [&](const TableView& tv, int b, int e) {
                    for (int q = b; q < e; ++q) {
                        if (tv.t->flags[q] & 512) continue;               // Read_IsQCFail
                        src.push_back((int32_t)(tv.base + q));
                        roff.push_back(roff.back() + tv.rlen(q));
                    }
                };
                take(r.samples[i].reads, p.gs, p.ge);
                if (o.assembleBadReads) take(r.samples[i].bad, p.bs, p.be);
                if (o.assembleBrokenPairs) take(r.samples[i].broken, p.ks, p.ke);
            }
            rbegin.push_back((int32_t)src.size());
        }
    }
    const int nT = (int)tiles.size();
    if (nT > 0) {
        Layout L;
        L.add(z.as_ref, blob.size() + PLAT_BLOB_PAD); L.put(z.as_refoff, refoff); L.put(z.as_refstart, refstart); L.put(z.as_astart, astart);
        L.put(z.as_aend, aend); L.put(z.as_rbegin, rbegin); L.put(z.as_src, src); L.put(z.as_roff, roff);
        L.commit(z, z.a_asin);
        memcpy(z.as_ref.h, blob.data(), blob.size()); memset(z.as_ref.h + blob.size(), 0, PLAT_BLOB_PAD);
        L.upload(z, z.a_asin);
        const size_t nR = src.size(), nb = (size_t)roff.back();
        z.as_seq.reserve(z.ctx, nb + PLAT_BLOB_PAD, false, true, z.stream); z.as_qual.reserve(z.ctx, nb + PLAT_BLOB_PAD, false, true, z.stream);
        z.as_pos.reserve(z.ctx, nR + 1, false); z.as_end.reserve(z.ctx, nR + 1, false); z.as_flags.reserve(z.ctx, nR + 1, false); z.as_mapq.reserve(z.ctx, nR + 1, false);
        if (nR) z.gatherReads((int64_t)nR, z.as_src.d, z.as_roff.d, z.as_seq.d, z.as_qual.d, z.as_pos.d, z.as_end.d, z.as_mapq.d, z.as_flags.d, "plat_gather_reads(assembler)");
        plat_assembly_batch& ab = asmBatch;
        memset(&ab, 0, sizeof ab);
        ab.n_regions = nT; ab.n_reads = (int32_t)nR;
        ab.ref_seq = z.as_ref.d; ab.ref_off = z.as_refoff.d; ab.ref_start = z.as_refstart.d; ab.assem_start = z.as_astart.d; ab.assem_end = z.as_aend.d;
        ab.reg_read_begin = z.as_rbegin.d; ab.read_seq = z.as_seq.d; ab.read_qual = z.as_qual.d; ab.read_off = z.as_roff.d;
        memset(&asmHints, 0, sizeof asmHints);
        for (int g = 0; g < nT; ++g) {
            const int64_t rl = refoff[(size_t)g + 1] - refoff[(size_t)g], nr = rbegin[(size_t)g + 1] - rbegin[(size_t)g];
            const int64_t bytes = roff[(size_t)rbegin[(size_t)g + 1]] - roff[(size_t)rbegin[(size_t)g]];
            asmHints.max_ref_len = std::max<int32_t>(asmHints.max_ref_len, (int32_t)rl);
            asmHints.max_reads_per_region = std::max<int32_t>(asmHints.max_reads_per_region, (int32_t)nr);
            asmHints.max_positions = std::max<int64_t>(asmHints.max_positions, rl + 2 + bytes + 2 * nr);
        }
        asmN = nT;
        assembleEnqueue();
    }
    std::lock_guard<std::mutex> g(stMutex);
    st.seconds_assemble += secs(t0, Clock::now());
}

inline void Chunk::assembleEnqueue() {
    Slot& z = s;
    const int nT = asmN;
    Layout LO;
    LO.add(z.as_cnt, (size_t)nT); LO.add(z.as_status, (size_t)nT); LO.add(z.as_vpos, (size_t)nT * asmMaxVars); LO.add(z.as_nrem, (size_t)nT * asmMaxVars);
    LO.add(z.as_nadd, (size_t)nT * asmMaxVars); LO.add(z.as_off, (size_t)nT * asmMaxVars); LO.add(z.as_blob, (size_t)nT * asmBlob);
    LO.commit(z, z.a_asout);
    ck(plat_assemble_batch_async(z.ctx, &asmBatch, &asmHints, o.assemblerKmerSize, o.minBaseQual, o.minReads * o.minBaseQual, o.noCycles, asmMaxVars, asmBlob,
                                 z.as_cnt.d, z.as_vpos.d, z.as_nrem.d, z.as_nadd.d, z.as_off.d, z.as_blob.d, z.as_status.d, z.stream), "plat_assemble_batch_async");
    LO.download(z, z.a_asout);
}

inline void Chunk::assembleCollect() {
    if (!o.assemble || asmN == 0) return;
    Slot& z = s;
    const auto t0 = Clock::now();
    const int nT = asmN;
    const std::vector<Tile>& tiles = asmTiles;
    {
        for (;;) {                                                       // room per tile grows until every tile's variants fit
            z.sync("assembler");                                         // (already over when the scan's wait covered it)
            bool over = false;
            for (int g = 0; g < nT; ++g) {
                if (z.as_status.h[g] == PLAT_ERR_OVERFLOW) over = true;
                else if (z.as_status.h[g] != 0) throw DeviceError(z.as_status.h[g], "plat_assemble_batch(tile)");
            }
            if (!over) break;
            if (asmMaxVars >= (1 << 14)) throw DeviceError(PLAT_ERR_OVERFLOW, "plat_assemble_batch(tile)");
            asmMaxVars *= 4; asmBlob *= 4;
            assembleEnqueue();
        }
        int64_t nv = 0;
        for (int g = 0; g < nT; ++g) {                                   // per tile in the reference's sorted() order (the device's), tile after tile
            RegionWork& r = *regions[(size_t)tiles[(size_t)g].region];
            const uint8_t* raw = z.as_blob.h + (size_t)g * (size_t)asmBlob;
            for (int i = 0; i < z.as_cnt.h[g]; ++i) {
                const size_t k = (size_t)g * (size_t)asmMaxVars + (size_t)i;
                const int off = z.as_off.h[k], nrem = z.as_nrem.h[k], nadd = z.as_nadd.h[k];
                r.asmVariants.push_back(r.pool.make(z.as_vpos.h[k], std::string((const char*)raw + off, (size_t)nrem),
                                                    std::string((const char*)raw + off + nrem, (size_t)nadd), 0, ASSEMBLER_VAR));
                ++nv;
            }
        }
        std::lock_guard<std::mutex> g(stMutex);
        st.n_assembly_tiles += nT; st.n_assembler_variants += nv;
    }
    std::lock_guard<std::mutex> g(stMutex);
    st.seconds_assemble += secs(t0, Clock::now());
}

}  // namespace plathost
