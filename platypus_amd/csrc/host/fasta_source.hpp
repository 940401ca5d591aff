// fasta_source.hpp -- plat_fasta_* (include/platypus_caller_fasta.h): the reference FASTA taken as the file's bytes and its .fai.  The
// index is parsed on the host by the rule's own line parse (csrc/fasta_rule.hpp, parse_fai_line); contigs (plat_fasta_load,
// plat_fasta_contig: whole-contig mode) and sequence windows (plat_fasta_get_sequences: getSequence) are fetched by ONE
// plat_fasta_fetch_batch per call on slot 0's stream with one wait -- the part of the file that holds the call's spans is uploaded, the
// offset of its first byte going into file_base.  PLAT_CALLER_HOST_FASTA=1 answers with the host twin (twinFetch: the rule's span, its
// byte map, one loop) instead.
// Included at the end of region_caller.cpp, after index_source.hpp.
#pragma once
#include "../../../include/platypus_caller_fasta.h"
#include "../fasta_rule.hpp"

// referenced weakly, as plat_index_query_batch (index_source.hpp): the CPU suite's stand-in device library predates it
#pragma weak plat_fasta_fetch_batch

struct plat_fasta {
    plat_caller* c = nullptr;
    const uint8_t* file = nullptr;
    int64_t fileLen = 0;
    struct Ref { std::string name; fasta::Entry e; };
    std::vector<Ref> refs;                                                // in file order; a repeated name keeps its first place and takes the later numbers
    std::unordered_map<std::string, int> tidOf;
    // what a load left: host memory (pinned where the device library pins) and its device copy, each with PLAT_BLOB_PAD zero bytes behind
    struct Loaded { uint8_t* host = nullptr; uint8_t* dev = nullptr; };
    std::vector<Loaded> blobs;
    struct Contig { bool loaded = false; const uint8_t* host = nullptr; const uint8_t* dev = nullptr; int64_t len = 0; };
    std::vector<Contig> contigs;                                          // [refs]
    std::vector<int64_t> first;                                           // the last plat_fasta_get_sequences' answer
    std::vector<uint8_t> bytes;
    std::vector<int32_t> status;
    ~plat_fasta() {
        plat_ctx* ctx = c ? c->slots[0]->ctx : nullptr;
        for (Loaded& b : blobs) { if (b.host) plat_host_free(ctx, b.host); if (b.dev) plat_free(ctx, b.dev); }
    }
};

namespace plathost {

struct FastaQuery { fasta::Entry e; int64_t beg, end; uint8_t mode; };

// the host twin of plat_fasta_fetch_batch over the whole file: every query's status, and its bytes appended to out
inline void twinFetch(const uint8_t* file, int64_t fileLen, const std::vector<FastaQuery>& qs, std::vector<int64_t>& first, std::vector<int32_t>& status, std::vector<uint8_t>& out)
{
    first.assign(qs.size() + 1, 0); status.assign(qs.size(), 0); out.clear();
    for (size_t q = 0; q < qs.size(); ++q) {
        const fasta::Span s = fasta::span_of(qs[q].e, qs[q].beg, qs[q].end, qs[q].mode, fileLen);
        status[q] = s.status;
        for (int64_t i = s.lo; i < s.hi; ++i) if (fasta::keeps(file[i])) out.push_back(fasta::upper(file[i]));
        first[q + 1] = (int64_t)out.size();
    }
}

// The queries on the device: the cut that holds their spans uploaded, one batch, one wait.  Returns the output blob on the device (dOut, owned
// by `dev`, capBytes + PLAT_BLOB_PAD bytes, the pad zeroed) with first / status on the host; the bytes are copied to hostOut when it is given
// (the same wait).  Every span is computed here first (the rule is the same code): the cut and an exact capacity need no second call.
inline uint8_t* deviceFetch(plat_fasta& R, FetchedDeviceBuffers& dev, const std::vector<FastaQuery>& qs, std::vector<int64_t>& first, std::vector<int32_t>& status,
                            uint8_t* hostOut, int64_t hostCap, int64_t* cutBytes, uint8_t* dOutGiven, int64_t* needBytes)
{
    Slot& z = *R.c->slots[0];
    void* st = z.stream;
    const size_t n = qs.size();
    int64_t lo = INT64_MAX, hi = 0, cap = 0;
    for (const FastaQuery& q : qs) {
        const fasta::Span s = fasta::span_of(q.e, q.beg, q.end, q.mode, R.fileLen);
        if (s.status != fasta::ST_OK || s.lo >= s.hi) continue;
        lo = std::min(lo, s.lo); hi = std::max(hi, s.hi); cap += s.hi - s.lo;
    }
    if (lo > hi) { lo = 0; hi = 0; }
    lo &= ~(int64_t)15;                                                   // (the cut begins at an aligned byte of the file: a span keeps its residue)
    if (needBytes) { *needBytes = cap; if (!dOutGiven) return nullptr; }
    plat_fasta_fetch_in in;
    memset(&in, 0, sizeof in);
    uint8_t* dFile = dev.alloc<uint8_t>((size_t)(hi - lo) + 16);
    if (hi > lo) ck(plat_memcpy_h2d(z.ctx, dFile, R.file + lo, (size_t)(hi - lo), st), "plat_memcpy_h2d");
    in.file = dFile; in.file_len = hi - lo; in.file_base = lo; in.file_size = R.fileLen; in.n_queries = (int64_t)n;
    std::vector<int64_t> a[6];
    std::vector<uint8_t> mode(n);
    for (auto& v : a) v.resize(n);
    for (size_t q = 0; q < n; ++q) {
        a[0][q] = qs[q].e.start_pos; a[1][q] = qs[q].e.line_len; a[2][q] = qs[q].e.full_len; a[3][q] = qs[q].e.seq_len; a[4][q] = qs[q].beg; a[5][q] = qs[q].end;
        mode[q] = qs[q].mode;
    }
    in.start_pos = dev.upload(a[0], st); in.line_len = dev.upload(a[1], st); in.full_len = dev.upload(a[2], st); in.seq_len = dev.upload(a[3], st);
    in.beg = dev.upload(a[4], st); in.end = dev.upload(a[5], st); in.mode = dev.upload(mode, st);
    plat_fasta_fetch_out o;
    memset(&o, 0, sizeof o);
    o.cap_bytes = cap;
    o.out_off = dev.alloc<int64_t>(n + 1); o.out_status = dev.alloc<int32_t>(n); o.totals = dev.alloc<int64_t>(PLAT_FASTA_STATUS_WORDS);
    o.out = dOutGiven ? dOutGiven : dev.alloc<uint8_t>((size_t)cap + PLAT_BLOB_PAD);
    ck(plat_memset(z.ctx, o.out + cap, 0, PLAT_BLOB_PAD, st), "plat_memset");
    ck(plat_fasta_fetch_batch(z.ctx, &in, &o, st), "plat_fasta_fetch_batch");
    int64_t totals[PLAT_FASTA_STATUS_WORDS] = {0};
    first.assign(n + 1, 0); status.assign(n, 0);
    dev.download(totals, o.totals, (size_t)PLAT_FASTA_STATUS_WORDS, st);
    dev.download(first, o.out_off, st); dev.download(status, o.out_status, st);
    if (hostOut && cap > 0) dev.download(hostOut, o.out, (size_t)std::min(cap, hostCap), st);
    ck(plat_stream_sync(z.ctx, st), "plat_stream_sync");                    // the one wait
    if (totals[0] != 0) throw DeviceError((int)totals[0], "plat_fasta_fetch_batch");
    if (first[n] != totals[1] || first[n] > cap) throw DeviceError(PLAT_ERR_INVALID, "plat_fasta_fetch_batch (counts that do not sum to the bytes)");
    if (cutBytes) *cutBytes = hi - lo;
    return o.out;
}

inline std::string fastaWhyNot(int32_t st)
{
    return st == fasta::ST_ZERO_LINE ? "its index line has LineLength 0, which the reference divides by" :
           st == fasta::ST_INDEX_ERROR ? "end lies in front of beg (the reference's IndexError)" : "its index line's numbers leave 63 bits";
}

// contigs `tids` (all of them: empty) fetched whole, into memory the object keeps
inline int loadContigs(plat_fasta& R, const std::vector<int>& tidsIn, plat_fasta_info* info)
{
    const auto t0 = Clock::now();
    if (info) memset(info, 0, sizeof *info);
    plat_caller* c = R.c;
    const bool onHost = Switches::read().hostFasta;
    if (!onHost) { const int rc = needsEntryPoints(c, "plat_fasta_load", {(const void*)plat_fasta_fetch_batch}, "plat_fasta_fetch_batch"); if (rc != PLAT_OK) return rc; }
    std::vector<int> tids;
    if (tidsIn.empty()) { for (size_t t = 0; t < R.refs.size(); ++t) tids.push_back((int)t); }
    else tids = tidsIn;
    std::vector<FastaQuery> qs;
    for (int t : tids) {
        if (t < 0 || (size_t)t >= R.refs.size()) { c->lastError = "plat_fasta_load: tid " + std::to_string(t) + " lies outside the index's " + std::to_string(R.refs.size()) + " contigs"; return PLAT_ERR_INVALID; }
        const int32_t es = fasta::span_of(R.refs[(size_t)t].e, 0, 0, fasta::MODE_CONTIG, R.fileLen).status;
        if (es != fasta::ST_OK) { c->lastError = "plat_fasta_load: contig " + R.refs[(size_t)t].name + " cannot be fetched: " + fastaWhyNot(es); return PLAT_ERR_BAD_INPUT; }
        qs.push_back(FastaQuery{R.refs[(size_t)t].e, 0, 0, fasta::MODE_CONTIG});
    }
    Slot& z = *c->slots[0];
    std::vector<int64_t> first;
    std::vector<int32_t> status;
    plat_fasta::Loaded blob;
    int64_t cut = 0, total = 0;
    if (onHost) {
        std::vector<uint8_t> out;
        twinFetch(R.file, R.fileLen, qs, first, status, out);
        total = (int64_t)out.size();
        ck(plat_host_alloc(z.ctx, (size_t)total + PLAT_BLOB_PAD, (void**)&blob.host), "plat_host_alloc");
        R.blobs.push_back(blob);
        if (total) memcpy(blob.host, out.data(), (size_t)total);
        memset(blob.host + total, 0, PLAT_BLOB_PAD);
    } else {
        FetchedDeviceBuffers dev(z);
        deviceFetch(R, dev, qs, first, status, nullptr, 0, nullptr, nullptr, &total);        // (the spans' bytes: the capacity)
        ck(plat_malloc(z.ctx, (size_t)total + PLAT_BLOB_PAD, (void**)&blob.dev), "plat_malloc");
        R.blobs.push_back(blob);                                           // (owned from here on, whatever is thrown)
        ck(plat_host_alloc(z.ctx, (size_t)total + PLAT_BLOB_PAD, (void**)&R.blobs.back().host), "plat_host_alloc");
        blob = R.blobs.back();
        memset(blob.host, 0, (size_t)total + PLAT_BLOB_PAD);
        deviceFetch(R, dev, qs, first, status, blob.host, total, &cut, blob.dev, nullptr);
    }
    for (size_t k = 0; k < tids.size(); ++k) {
        plat_fasta::Contig& g = R.contigs[(size_t)tids[k]];
        g.loaded = true; g.host = blob.host + first[k]; g.dev = blob.dev ? blob.dev + first[k] : nullptr; g.len = first[k + 1] - first[k];
    }
    if (info) { info->queries = (int64_t)tids.size(); info->file_bytes = cut; info->out_bytes = first[tids.size()]; info->device_calls = onHost ? 0 : 1; info->seconds = secs(t0, Clock::now()); }
    return PLAT_OK;
}

inline int getSequences(plat_fasta& R, int n, const int32_t* tid, const int64_t* beg, const int64_t* end, plat_fasta_info* info)
{
    const auto t0 = Clock::now();
    if (info) memset(info, 0, sizeof *info);
    plat_caller* c = R.c;
    R.first.assign((size_t)n + 1, 0); R.bytes.clear(); R.status.assign((size_t)n, 0);
    const bool onHost = Switches::read().hostFasta;
    if (!onHost) { const int rc = needsEntryPoints(c, "plat_fasta_get_sequences", {(const void*)plat_fasta_fetch_batch}, "plat_fasta_fetch_batch"); if (rc != PLAT_OK) return rc; }
    std::vector<FastaQuery> qs;
    for (int q = 0; q < n; ++q) {
        if (tid[q] < 0 || (size_t)tid[q] >= R.refs.size()) {
            c->lastError = "plat_fasta_get_sequences: query " + std::to_string(q) + " asks for tid " + std::to_string(tid[q]) + ", outside the index's " + std::to_string(R.refs.size()) + " contigs";
            return PLAT_ERR_INVALID;
        }
        qs.push_back(FastaQuery{R.refs[(size_t)tid[q]].e, beg[q], end[q], fasta::MODE_SEQUENCE});
    }
    int64_t cut = 0;
    if (onHost) twinFetch(R.file, R.fileLen, qs, R.first, R.status, R.bytes);
    else if (n > 0) {
        FetchedDeviceBuffers dev(*c->slots[0]);
        int64_t total = 0;
        deviceFetch(R, dev, qs, R.first, R.status, nullptr, 0, nullptr, nullptr, &total);
        R.bytes.resize((size_t)total);
        uint8_t* dOut = dev.alloc<uint8_t>((size_t)total + PLAT_BLOB_PAD);
        deviceFetch(R, dev, qs, R.first, R.status, R.bytes.data(), total, &cut, dOut, nullptr);
        R.bytes.resize((size_t)R.first[(size_t)n]);
    }
    if (info) { info->queries = n; info->file_bytes = cut; info->out_bytes = R.first[(size_t)n]; info->device_calls = onHost || n == 0 ? 0 : 1; info->seconds = secs(t0, Clock::now()); }
    return PLAT_OK;
}

// the .fai's lines by the rule's parse; 0, or PLAT_ERR_BAD_INPUT with the line named
inline int parseFai(plat_fasta& R, const uint8_t* fai, int64_t len, int parseNCBI, std::string& why)
{
    int64_t lineNo = 0;
    for (int64_t at = 0; at < len;) {
        int64_t nl = at;
        while (nl < len && fai[nl] != '\n') ++nl;
        const int64_t next = nl < len ? nl + 1 : len;                      // (the file iterator's line: through its '\n')
        ++lineNo;
        fasta::FaiLine L;
        const int rc = fasta::parse_fai_line(fai + at, next - at, parseNCBI, &L);
        const std::string where = "plat_fasta_open: line " + std::to_string(lineNo) + " of the index ";
        if (rc == fasta::FAI_NO_NAME) { why = where + "has no name in its first field (the reference raises IndexError; a blank line is such a line)"; return PLAT_ERR_BAD_INPUT; }
        if (rc == fasta::FAI_FEW_FIELDS) { why = where + "has fewer than five tab-separated fields (the reference raises IndexError)"; return PLAT_ERR_BAD_INPUT; }
        if (L.e.start_pos < 0 || L.e.line_len < 0 || L.e.seq_len < 0) { why = where + "has a negative StartPos, LineLength or SeqLength (the reference would seek to a negative offset)"; return PLAT_ERR_BAD_INPUT; }
        if (L.e.full_len < L.e.line_len) { why = where + "has FullLineLength < LineLength (the reference would seek backwards, to a negative offset in the end)"; return PLAT_ERR_BAD_INPUT; }
        const std::string name((const char*)fai + at + L.name_at, (size_t)L.name_len);
        const auto it = R.tidOf.find(name);
        if (it != R.tidOf.end()) R.refs[(size_t)it->second].e = L.e;       // (theDict[seqName] = ...: the later line's numbers)
        else { R.tidOf.emplace(name, (int)R.refs.size()); R.refs.push_back(plat_fasta::Ref{name, L.e}); }
        at = next;
    }
    R.contigs.assign(R.refs.size(), plat_fasta::Contig());
    return PLAT_OK;
}

}  // namespace plathost

CALLER_EXPORT int plat_fasta_open(plat_caller* c, const uint8_t* file_bytes, int64_t file_len, const uint8_t* fai_bytes, int64_t fai_len, int parseNCBI, plat_fasta** out)
{
    if (!c || !out || file_len < 0 || fai_len < 0 || (file_len > 0 && !file_bytes) || (fai_len > 0 && !fai_bytes)) return PLAT_ERR_INVALID;
    *out = nullptr;
    return guardedEntry(c, "plat_fasta_open", [&] {
        std::unique_ptr<plat_fasta> R(new plat_fasta);
        R->file = file_bytes; R->fileLen = file_len;
        const int rc = parseFai(*R, fai_bytes, fai_len, parseNCBI, c->lastError);
        if (rc != PLAT_OK) return rc;
        R->c = c;                                                          // (from here on the destructor frees through the caller's context)
        *out = R.release();
        return (int)PLAT_OK;
    });
}

CALLER_EXPORT int plat_fasta_close(plat_fasta* ref) { if (!ref) return PLAT_ERR_INVALID; delete ref; return PLAT_OK; }
CALLER_EXPORT int plat_fasta_n_refs(const plat_fasta* ref) { return ref ? (int)ref->refs.size() : PLAT_ERR_INVALID; }
CALLER_EXPORT int plat_fasta_ref(const plat_fasta* ref, int i, const char** name, int64_t* seq_len)
{
    if (!ref || i < 0 || (size_t)i >= ref->refs.size() || !name || !seq_len) return PLAT_ERR_INVALID;
    *name = ref->refs[(size_t)i].name.c_str(); *seq_len = ref->refs[(size_t)i].e.seq_len;
    return PLAT_OK;
}
CALLER_EXPORT int plat_fasta_ref_line(const plat_fasta* ref, int i, int64_t* start_pos, int64_t* line_len, int64_t* full_line_len)
{
    if (!ref || i < 0 || (size_t)i >= ref->refs.size() || !start_pos || !line_len || !full_line_len) return PLAT_ERR_INVALID;
    const fasta::Entry& e = ref->refs[(size_t)i].e;
    *start_pos = e.start_pos; *line_len = e.line_len; *full_line_len = e.full_len;
    return PLAT_OK;
}
CALLER_EXPORT int plat_fasta_tid(const plat_fasta* ref, const char* name)
{
    if (!ref || !name) return -1;
    const auto it = ref->tidOf.find(name);
    return it == ref->tidOf.end() ? -1 : it->second;
}
CALLER_EXPORT int64_t plat_fasta_total_length(const plat_fasta* ref)
{
    int64_t sum = 0;
    if (ref) for (const plat_fasta::Ref& r : ref->refs) sum += r.e.seq_len;
    return sum;
}

CALLER_EXPORT int plat_fasta_load(plat_fasta* ref, const int32_t* tids, int n, plat_fasta_info* info)
{
    if (!ref || n < 0 || (n > 0 && !tids)) return PLAT_ERR_INVALID;
    return guardedEntry(ref->c, "plat_fasta_load", [&] { return loadContigs(*ref, std::vector<int>(tids, tids + n), info); });
}

CALLER_EXPORT int plat_fasta_contig(plat_fasta* ref, int tid, const uint8_t** host_seq, const uint8_t** dev_seq, int64_t* len)
{
    if (!ref || !host_seq || !dev_seq || !len) return PLAT_ERR_INVALID;
    *host_seq = nullptr; *dev_seq = nullptr; *len = 0;
    if (tid < 0 || (size_t)tid >= ref->refs.size()) {
        ref->c->lastError = "plat_fasta_contig: tid " + std::to_string(tid) + " lies outside the index's " + std::to_string(ref->refs.size()) + " contigs";
        return PLAT_ERR_INVALID;
    }
    if (!ref->contigs[(size_t)tid].loaded) {
        const int rc = guardedEntry(ref->c, "plat_fasta_contig", [&] { return loadContigs(*ref, std::vector<int>{tid}, nullptr); });
        if (rc != PLAT_OK) {
            const std::string from = "plat_fasta_load";                    // (the message names the entry point that was called)
            if (ref->c->lastError.compare(0, from.size(), from) == 0) ref->c->lastError = "plat_fasta_contig" + ref->c->lastError.substr(from.size());
            return rc;
        }
    }
    const plat_fasta::Contig& g = ref->contigs[(size_t)tid];
    *host_seq = g.host; *dev_seq = g.dev; *len = g.len;
    return PLAT_OK;
}

CALLER_EXPORT int plat_fasta_get_sequences(plat_fasta* ref, int n, const int32_t* tid, const int64_t* beg, const int64_t* end,
                                           const int64_t** first, const uint8_t** bytes, const int32_t** status, plat_fasta_info* info)
{
    if (!ref || n < 0 || (n > 0 && (!tid || !beg || !end)) || !first || !bytes || !status) return PLAT_ERR_INVALID;
    *first = nullptr; *bytes = nullptr; *status = nullptr;
    const int rc = guardedEntry(ref->c, "plat_fasta_get_sequences", [&] { return getSequences(*ref, n, tid, beg, end, info); });
    if (rc != PLAT_OK) return rc;
    ref->bytes.reserve(1);                                                 // (a pointer for an empty answer too)
    *first = ref->first.data(); *bytes = ref->bytes.data(); *status = ref->status.data();
    return PLAT_OK;
}

CALLER_EXPORT int plat_fasta_get_character(const plat_fasta* ref, int tid, int64_t pos, uint8_t* out, int32_t* n_out)
{
    if (!ref || !out || !n_out || tid < 0 || (size_t)tid >= ref->refs.size()) return PLAT_ERR_INVALID;
    int32_t st = 0;
    const int ch = fasta::character_at(ref->refs[(size_t)tid].e, pos, ref->file, ref->fileLen, &st);
    *out = ch < 0 ? 0 : (uint8_t)ch; *n_out = ch < 0 ? 0 : 1;
    if (st != fasta::ST_OK) { ref->c->lastError = "plat_fasta_get_character: contig " + ref->refs[(size_t)tid].name + ": " + plathost::fastaWhyNot(st); return PLAT_ERR_BAD_INPUT; }
    return PLAT_OK;
}
