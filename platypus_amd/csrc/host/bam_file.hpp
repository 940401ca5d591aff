// bam_file.hpp -- plat_bam_file_*, plat_bam_files_plan, plat_bam_files_fetch_plan and plat_call_bam_files (include/platypus_caller_bamfile.h):
// a BAM file and its .bai opened once -- the header inflated on the host as far as it reaches (bgzf_blocks.hpp's block list and host
// inflate over a growing prefix of the file), its text read by the rule of Samfile.header and getSampleNamesAndLoadIterators (bamhdr::
// below, the standard library alone), the .bai through plat_index_open --, loadBAMData's choice between one stream per sample and the
// split by read group, per file one index fetch for all regions of a call (fetchIndexChunks, index_source.hpp: the queries in one batch,
// every chunk cut out of the file), and from there plat_call_bgzf_regions or plat_call_bgzf_regions_rg on those structures
// (callBamFilesWith: the frame plat_call_bam_files_mates of bam_mates.hpp shares, as it shares the entry points' argument checks).
// Included at the end of region_caller.cpp, after index_source.hpp.
#pragma once
#include <algorithm>
#include <map>
#include "../../../include/platypus_caller_bamfile.h"

namespace plathost {
namespace bamhdr {

// what reading one header leaves: the read groups entered into samplesByID, the samples added to the sample list, and whether it raised
struct HeaderSamples {
    std::vector<std::pair<std::string, std::string>> groups;              // (ID, SM) in header order
    std::vector<std::string> samples;                                     // distinct SM in first-seen order; the file name's when raised
    bool raised = false;
    std::string why;
    // what getRegions reads (platypusutils.pyx:1002-1003, :1028-1030): (SN, LN) of the @SQ lines; sqRaised when that read raises -- the
    // getter itself, no @SQ line, or one without SN or LN
    std::vector<std::pair<std::string, long long>> sq;
    bool sqRaised = false;
};

inline bool pySpace(char ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r' || ch == '\v' || ch == '\f'; }
// int(value) of Python 2 for a str: blanks around an optional sign and at least one digit
inline bool pyIntParses(const std::string& v)
{
    size_t a = 0, b = v.size();
    while (a < b && pySpace(v[a])) ++a;
    while (b > a && pySpace(v[b - 1])) --b;
    if (a < b && (v[a] == '+' || v[a] == '-')) ++a;
    if (a >= b) return false;
    for (size_t i = a; i < b; ++i) if (v[i] < '0' || v[i] > '9') return false;
    return true;
}
// VALID_HEADER_FIELDS (htslibWrapper.pyx:26-29); CO has none: its lines are kept whole
inline const char* const* validFields(const std::string& record)
{
    static const char* const HD[] = {"VN", "SO", "GO", nullptr};
    static const char* const SQ[] = {"SN", "LN", "AH", "AS", "M5", "UR", "SP", nullptr};
    static const char* const RG[] = {"ID", "SM", "LB", "DS", "PU", "PI", "CN", "DT", "PL", "PG", nullptr};
    static const char* const PG[] = {"ID", "VN", "CL", "PN", "PP", "DS", nullptr};
    static const char* const CO[] = {nullptr};
    return record == "HD" ? HD : record == "SQ" ? SQ : record == "RG" ? RG : record == "PG" ? PG : record == "CO" ? CO : nullptr;
}

// file_name.split("/")[-1][0:-4]
inline std::string sampleOfFileName(const std::string& fileName)
{
    const size_t slash = fileName.rfind('/');
    const std::string last = slash == std::string::npos ? fileName : fileName.substr(slash + 1);
    return last.size() > 4 ? last.substr(0, last.size() - 4) : std::string();
}

// htslibWrapper.pyx:247-289 as far as platypusutils.pyx:114-147 reads its result
inline HeaderSamples samplesOfHeader(const std::string& text, const std::string& fileName)
{
    HeaderSamples out;
    struct Group { bool hasId = false, hasSm = false; std::string id, sm; };
    std::vector<Group> rgs;
    bool seenHD = false, parsed = false;
    auto raise = [&](const std::string& why) {
        out.raised = true; out.why = why;
        if (!parsed) { out.sq.clear(); out.sqRaised = true; }
        out.samples.assign(1, sampleOfFileName(fileName));
        return out;
    };
    for (size_t at = 0; at <= text.size();) {
        size_t eol = text.find('\n', at);
        if (eol == std::string::npos) eol = text.size();
        const std::string line = text.substr(at, eol - at);
        at = eol + 1;
        if (std::all_of(line.begin(), line.end(), pySpace)) continue;
        if (line[0] != '@') return raise("Header line without '@': '" + line + "'");
        std::vector<std::string> fields;
        for (size_t p = 1;;) {
            const size_t tab = line.find('\t', p);
            fields.push_back(line.substr(p, tab == std::string::npos ? std::string::npos : tab - p));
            if (tab == std::string::npos) break;
            p = tab + 1;
        }
        const std::string& record = fields[0];
        const char* const* valid = validFields(record);
        if (!valid) return raise("header line with invalid type '" + record + "': '" + line + "'");
        if (record == "CO") continue;
        Group g;
        bool hasSn = false, hasLn = false;
        std::string sn;
        long long ln = 0;
        for (size_t k = 1; k < fields.size(); ++k) {
            const size_t colon = fields[k].find(':');
            if (colon == std::string::npos) return raise("need more than 1 value to unpack");
            const std::string key = fields[k].substr(0, colon), value = fields[k].substr(colon + 1);
            bool known = false;
            for (const char* const* v = valid; *v; ++v) known = known || key == *v;
            if (!known) return raise("unknown field code '" + key + "' in record '" + record + "'");
            if (record == "SQ" && key == "LN" && !pyIntParses(value)) return raise("invalid literal for int() with base 10: '" + value + "'");
            if (record == "SQ" && key == "SN") { hasSn = true; sn = value; }
            if (record == "SQ" && key == "LN") { hasLn = true; ln = strtoll(value.c_str(), nullptr, 10); }
            if (record == "RG" && key == "ID") { g.hasId = true; g.id = value; }
            if (record == "RG" && key == "SM") { g.hasSm = true; g.sm = value; }
        }
        if (record == "HD") { if (seenHD) return raise("multiple 'HD' lines are not permitted"); seenHD = true; }
        if (record == "RG") rgs.push_back(g);
        if (record == "SQ") { if (hasSn && hasLn) out.sq.emplace_back(sn, ln); else out.sqRaised = true; }
    }
    parsed = true;
    if (out.sqRaised || out.sq.empty()) { out.sq.clear(); out.sqRaised = true; }
    if (rgs.empty()) return raise("'RG'");                                // (theHeader['RG']: KeyError)
    for (const Group& g : rgs) {
        if (!g.hasSm) return raise("'SM'");
        if (std::find(out.samples.begin(), out.samples.end(), g.sm) == out.samples.end()) out.samples.push_back(g.sm);
    }
    for (const Group& g : rgs) {
        if (!g.hasId) return raise("'ID'");                               // (the groups in front of it stay entered)
        out.groups.emplace_back(g.id, g.sm);
    }
    return out;
}

// loadBAMData's decision over the files' samples (platypusutils.pyx:462-484) and the merged path's table
struct FilesPlan {
    int mode = PLAT_BAM_FILES_MERGED;
    std::vector<std::string> samples;                                     // sorted(set(samples))
    std::vector<int32_t> sampleFile;                                      // pre-split
    std::vector<std::string> groupId;                                     // merged: first-seen order, the last SM of an ID
    std::vector<int32_t> groupSample;
};
// 0, or the sample (index into plan.samples) that not exactly one file holds: the reference's failed assertion
inline int planFiles(const std::vector<const HeaderSamples*>& files, FilesPlan& plan)
{
    for (const HeaderSamples* h : files) plan.samples.insert(plan.samples.end(), h->samples.begin(), h->samples.end());
    std::sort(plan.samples.begin(), plan.samples.end());
    plan.samples.erase(std::unique(plan.samples.begin(), plan.samples.end()), plan.samples.end());
    if (plan.samples.size() == files.size()) {
        plan.mode = PLAT_BAM_FILES_PRESPLIT;
        for (size_t s = 0; s < plan.samples.size(); ++s) {
            const std::string& sample = plan.samples[s];
            int found = -1, n = 0;
            for (size_t f = 0; f < files.size(); ++f) {
                const HeaderSamples& h = *files[f];
                // `sample in samplesByBAM[x]`: a list of samples, or -- where the header raised -- the one name, a str
                const bool in = h.raised ? h.samples[0].find(sample) != std::string::npos : std::find(h.samples.begin(), h.samples.end(), sample) != h.samples.end();
                if (in) { found = (int)f; ++n; }
            }
            if (n != 1) return (int)s + 1;
            plan.sampleFile.push_back(found);
        }
        return 0;
    }
    std::map<std::string, size_t> at;
    std::vector<std::string> sm;
    for (const HeaderSamples* h : files)
        for (const auto& g : h->groups) {
            const auto it = at.find(g.first);
            if (it == at.end()) { at.emplace(g.first, plan.groupId.size()); plan.groupId.push_back(g.first); sm.push_back(g.second); }
            else sm[it->second] = g.second;
        }
    std::vector<std::string> ids;
    for (size_t k = 0; k < sm.size(); ++k) {
        const auto it = std::lower_bound(plan.samples.begin(), plan.samples.end(), sm[k]);
        if (it == plan.samples.end() || *it != sm[k]) continue;         // (entered in front of an @RG line without ID: its sample is not one of the call's)
        ids.push_back(plan.groupId[k]); plan.groupSample.push_back((int32_t)(it - plan.samples.begin()));
    }
    plan.groupId.swap(ids);
    return 0;
}

}  // namespace bamhdr

// the inflated front of a BAM file, grown block by block as the header's counts ask for more
struct BamHeaderBytes {
    const uint8_t* data; int64_t len;
    int64_t at = 0;                                                       // compressed bytes inflated so far
    std::vector<uint8_t> buf;
    BamHeaderBytes(const uint8_t* d, int64_t l) : data(d), len(l) {}
    // 0: buf holds `need` bytes; 1: no BGZF block at `at`, or one that does not inflate; 2: the file ends first
    int ensure(uint64_t need)
    {
        while (buf.size() < need) {
            if (at >= len) return 2;
            plat_bgzf_chunk ch;
            memset(&ch, 0, sizeof ch);
            ch.data = data + at; ch.data_len = len - at; ch.end_coffset = -1;
            int64_t covered = 0;
            uint64_t got = 0;
            const uint64_t want = need - buf.size();
            walkBgzfChain(ch, [&](int64_t, const bgzf::BlockHead& h) { covered = h.payload + h.payload_len + 8; got += h.isize; return got < want; });
            if (covered == 0) return 1;
            ch.data_len = covered;
            std::string why;
            BgzfBlockList L("plat_bam_file_open", [](const BgzfChunkAt&) { return std::string(); }, false, why);
            std::vector<uint8_t> part;
            if (L.add(0, 0, 0, ch) != PLAT_OK || L.inflateOnHost(part) >= 0) return 1;
            buf.insert(buf.end(), part.begin(), part.end());
            at += covered;
        }
        return 0;
    }
    int32_t i32(uint64_t p) const { int32_t v; memcpy(&v, buf.data() + p, 4); return v; }
};

}  // namespace plathost

struct plat_bamfile {
    plat_caller* c = nullptr;
    const uint8_t* data = nullptr;
    int64_t len = 0;
    std::string fileName, text;
    std::vector<std::string> refName;
    std::vector<int64_t> refLen;
    std::unordered_map<std::string, int> tidOf;                           // (the first of equal names)
    plathost::bamhdr::HeaderSamples header;
    plat_index* index = nullptr;
    ~plat_bamfile() { if (index) plat_index_close(index); }
};

struct plat_bam_plan_impl : plat_bam_plan {
    plathost::bamhdr::FilesPlan P;
    std::vector<const char*> names, ids;
};
struct plat_bam_fetch_plan_impl : plat_bam_fetch_plan {
    std::vector<plat_bam_fetch> F;
    std::vector<std::vector<plat_bgzf_chunk>> chunks;                     // per fetch
};

CALLER_EXPORT int plat_bam_file_open(plat_caller* c, const uint8_t* data, int64_t data_len, const uint8_t* bai, size_t bai_len, const char* file_name,
                                     plat_bamfile** out)
{
    if (!c || !out || data_len < 0 || (data_len > 0 && !data) || (bai_len > 0 && !bai) || !file_name) return PLAT_ERR_INVALID;
    *out = nullptr;
    return guardedEntry(c, "plat_bam_file_open", [&] {
        std::unique_ptr<plat_bamfile> B(new plat_bamfile);
        B->c = c; B->data = data; B->len = data_len; B->fileName = file_name;
        BamHeaderBytes H(data, data_len);
        auto refuse = [&](int how, const char* what) {
            c->lastError = how == 1 ? std::string("plat_bam_file_open: the file's bytes are no BGZF stream that inflates (bad magic, no BC subfield, an invalid deflate stream or a CRC32 mismatch at offset ") +
                                          std::to_string(H.at) + ")"
                                    : std::string("plat_bam_file_open: ") + what;
            return (int)PLAT_ERR_BAD_INPUT;
        };
        int how;
        if ((how = H.ensure(12)) != 0) return refuse(how, "the file ends before the BAM magic and l_text");
        if (memcmp(H.buf.data(), "BAM\1", 4) != 0) return refuse(0, "the inflated bytes do not begin with BAM\\1 (a bad magic)");
        const int64_t lText = H.i32(4);
        if (lText < 0) return refuse(0, "l_text is negative");
        if ((how = H.ensure(12 + (uint64_t)lText)) != 0) return refuse(how, "l_text runs past the inflated bytes");
        B->text.assign((const char*)H.buf.data() + 8, (size_t)lText);
        B->text.resize(strlen(B->text.c_str()));                          // (Samfile.text: a C string of the l_text bytes)
        const int64_t nRef = H.i32(8 + (uint64_t)lText);
        if (nRef < 0) return refuse(0, "n_ref is negative");
        uint64_t p = 12 + (uint64_t)lText;
        for (int64_t t = 0; t < nRef; ++t) {
            if ((how = H.ensure(p + 4)) != 0) return refuse(how, "n_ref runs past the inflated bytes");
            const int64_t lName = H.i32(p);
            if (lName < 0) return refuse(0, "an l_name is negative");
            if ((how = H.ensure(p + 8 + (uint64_t)lName)) != 0) return refuse(how, "an l_name runs past the inflated bytes");
            std::string name((const char*)H.buf.data() + p + 4, (size_t)lName);
            name.resize(strlen(name.c_str()));
            B->tidOf.emplace(name, (int)t);
            B->refName.push_back(std::move(name));
            B->refLen.push_back(H.i32(p + 4 + (uint64_t)lName));
            p += 8 + (uint64_t)lName;
        }
        B->header = bamhdr::samplesOfHeader(B->text, B->fileName);
        int rc = plat_index_open(c, bai, bai_len, PLAT_INDEX_BAI, &B->index);
        if (rc != PLAT_OK) { c->lastError = "plat_bam_file_open: the .bai: " + c->lastError; return rc; }
        if (plat_index_n_refs(B->index) != (int)nRef) {
            c->lastError = "plat_bam_file_open: the .bai holds " + std::to_string(plat_index_n_refs(B->index)) + " references, the file's header " + std::to_string(nRef);
            return (int)PLAT_ERR_BAD_INPUT;
        }
        *out = B.release();
        return (int)PLAT_OK;
    });
}

CALLER_EXPORT int plat_bam_file_close(plat_bamfile* f) { if (!f) return PLAT_ERR_INVALID; delete f; return PLAT_OK; }
CALLER_EXPORT int plat_bam_file_n_refs(const plat_bamfile* f) { return f ? (int)f->refName.size() : PLAT_ERR_INVALID; }
CALLER_EXPORT const char* plat_bam_file_ref_name(const plat_bamfile* f, int tid) { return f && tid >= 0 && (size_t)tid < f->refName.size() ? f->refName[(size_t)tid].c_str() : nullptr; }
CALLER_EXPORT int64_t plat_bam_file_ref_len(const plat_bamfile* f, int tid) { return f && tid >= 0 && (size_t)tid < f->refLen.size() ? f->refLen[(size_t)tid] : -1; }
CALLER_EXPORT int plat_bam_file_tid(const plat_bamfile* f, const char* name)
{
    if (!f || !name) return -1;
    const auto it = f->tidOf.find(name);
    return it == f->tidOf.end() ? -1 : it->second;
}
CALLER_EXPORT const char* plat_bam_file_header_text(const plat_bamfile* f, int64_t* len)
{
    if (len) *len = f ? (int64_t)f->text.size() : 0;
    return f ? f->text.c_str() : nullptr;
}
CALLER_EXPORT int plat_bam_file_n_read_groups(const plat_bamfile* f) { return f ? (int)f->header.groups.size() : PLAT_ERR_INVALID; }
CALLER_EXPORT int plat_bam_file_read_group(const plat_bamfile* f, int i, const char** id, const char** sm)
{
    if (!f || !id || !sm || i < 0 || (size_t)i >= f->header.groups.size()) return PLAT_ERR_INVALID;
    *id = f->header.groups[(size_t)i].first.c_str(); *sm = f->header.groups[(size_t)i].second.c_str();
    return PLAT_OK;
}
CALLER_EXPORT int plat_bam_file_n_samples(const plat_bamfile* f) { return f ? (int)f->header.samples.size() : PLAT_ERR_INVALID; }
CALLER_EXPORT const char* plat_bam_file_sample(const plat_bamfile* f, int i) { return f && i >= 0 && (size_t)i < f->header.samples.size() ? f->header.samples[(size_t)i].c_str() : nullptr; }
CALLER_EXPORT int plat_bam_file_header_raised(const plat_bamfile* f, const char** why)
{
    if (why) *why = f ? f->header.why.c_str() : nullptr;
    return f ? (f->header.raised ? 1 : 0) : PLAT_ERR_INVALID;
}
CALLER_EXPORT int plat_bam_file_n_header_sq(const plat_bamfile* f) { return !f ? PLAT_ERR_INVALID : f->header.sqRaised ? -1 : (int)f->header.sq.size(); }
CALLER_EXPORT int plat_bam_file_header_sq(const plat_bamfile* f, int i, const char** name, int64_t* len)
{
    if (!f || !name || !len || i < 0 || (size_t)i >= f->header.sq.size()) return PLAT_ERR_INVALID;
    *name = f->header.sq[(size_t)i].first.c_str(); *len = f->header.sq[(size_t)i].second;
    return PLAT_OK;
}
CALLER_EXPORT plat_index* plat_bam_file_index(const plat_bamfile* f) { return f ? f->index : nullptr; }

namespace plathost {

// what every files entry point checks of its lists: the files all there and all of one caller, the regions pointer, chrom of every region
inline bool bamFilesArgsOk(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions, const plat_caller* c = nullptr)
{
    if (!files || n_files < 1 || n_regions < 0 || (n_regions > 0 && !regions)) return false;
    for (int f = 0; f < n_files; ++f) if (!files[f] || files[f]->c != (c ? c : files[0]->c)) return false;
    for (int k = 0; k < n_regions; ++k) if (!regions[k].chrom) return false;
    return true;
}
// A plan entry point: its plan cleared (as bamFilesCallArgsOk clears the text's outputs: in front of the other checks, so a call refused
// for another argument leaves them NULL / 0), its other arguments (argsOk) and its lists checked, the plan made under the guard.
template <class Impl, class Plan, class Make>
inline int bamFilesPlanEntry(const char* entry, Plan** plan, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions, bool argsOk, Make&& make)
{
    if (!plan) return PLAT_ERR_INVALID;
    *plan = nullptr;
    if (!argsOk || !bamFilesArgsOk(files, n_files, regions, n_regions)) return PLAT_ERR_INVALID;
    return guardedEntry(files[0]->c, entry, [&] {
        std::unique_ptr<Impl> I(new Impl);
        const int rc = make(*I);
        if (rc == PLAT_OK) *plan = I.release();
        return rc;
    });
}
// ... and what the two call entry points check: the text's outputs, cleared, the caller and the options
inline bool bamFilesCallArgsOk(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                               const plat_caller_options* options, char** out_text, size_t* out_len)
{
    if (!out_text || !out_len) return false;
    *out_text = nullptr; *out_len = 0;
    return c && options && bamFilesArgsOk(files, n_files, regions, n_regions, c);
}

inline int makeBamPlan(plat_bamfile* const* files, int n_files, plat_bam_plan_impl& I)
{
    std::vector<const bamhdr::HeaderSamples*> hs;
    for (int f = 0; f < n_files; ++f) hs.push_back(&files[f]->header);
    const int bad = bamhdr::planFiles(hs, I.P);
    if (bad) {
        files[0]->c->lastError = "plat_bam_files_plan: as many samples as files, but sample '" + I.P.samples[(size_t)bad - 1] +
                                 "' is not in exactly one file (the reference's assertion \"Something is screwy here\")";
        return PLAT_ERR_BAD_INPUT;
    }
    for (const std::string& s : I.P.samples) I.names.push_back(s.c_str());
    for (const std::string& s : I.P.groupId) I.ids.push_back(s.c_str());
    plat_bam_plan& p = I;
    memset(&p, 0, sizeof p);
    p.mode = I.P.mode; p.n_samples = (int32_t)I.names.size(); p.sample_names = I.names.data();
    p.sample_file = I.P.mode == PLAT_BAM_FILES_PRESPLIT ? I.P.sampleFile.data() : nullptr;
    p.groups.n_groups = (int32_t)I.ids.size(); p.groups.id = I.ids.data(); p.groups.sample = I.P.groupSample.data();
    return PLAT_OK;
}

inline int makeBamFetchPlan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions, plat_bam_fetch_plan_impl& I)
{
    const auto t0 = Clock::now();
    plat_caller* c = files[0]->c;
    plat_bam_fetch_plan& p = I;
    memset(&p, 0, sizeof p);
    I.F.assign((size_t)n_regions * (size_t)n_files, plat_bam_fetch{-1, 0, 0, 0, nullptr});
    I.chunks.assign(I.F.size(), {});
    for (int k = 0; k < n_regions; ++k) {
        const plat_bam_call_region& r = regions[k];
        const int32_t beg = std::max(r.start - 1, 0);
        if (beg >= r.end) {
            c->lastError = "plat_bam_files_fetch_plan: region " + std::to_string(k) + " (" + r.chrom + ":" + std::to_string(r.start) + "-" + std::to_string(r.end) +
                           ") is no window: max(start - 1, 0) >= end";
            return PLAT_ERR_INVALID;
        }
        for (int f = 0; f < n_files; ++f) { plat_bam_fetch& ft = I.F[(size_t)k * n_files + f]; ft.itr_beg = beg; ft.itr_end = r.end; ft.tid = plat_bam_file_tid(files[f], r.chrom); }
    }
    for (int f = 0; f < n_files; ++f) {
        std::vector<int32_t> tid, beg, end;
        std::vector<int> served;
        for (int k = 0; k < n_regions; ++k) {
            const plat_bam_fetch& ft = I.F[(size_t)k * n_files + f];
            if (ft.tid < 0) continue;                                      // (the reference's fetch raises: the file is empty for this region)
            tid.push_back(ft.tid); beg.push_back(ft.itr_beg); end.push_back(ft.itr_end); served.push_back(k);
        }
        plat_index_query_info qi;
        std::vector<std::vector<plat_bgzf_chunk>> chunks;
        const int rc = fetchIndexChunks(c, "plat_bam_files_fetch_plan", files[f]->data, files[f]->len, *files[f]->index, tid, beg, end,
                                        [&](size_t s) { return "region " + std::to_string(served[s]) + ", file " + std::to_string(f); }, chunks, &qi);
        if (rc != PLAT_OK) return rc;
        p.queries += qi.queries; p.handed_over += qi.handed_over; p.chunks += qi.chunks; p.device_calls += qi.device_calls;
        for (size_t s = 0; s < served.size(); ++s) I.chunks[(size_t)served[s] * n_files + f].swap(chunks[s]);
    }
    for (size_t i = 0; i < I.F.size(); ++i) { I.F[i].n_chunks = (int32_t)I.chunks[i].size(); I.F[i].chunks = I.chunks[i].data(); }
    p.n_regions = n_regions; p.n_files = n_files; p.fetches = I.F.data();
    p.seconds = secs(t0, Clock::now());
    return PLAT_OK;
}

}  // namespace plathost

CALLER_EXPORT int plat_bam_files_plan(plat_bamfile* const* files, int n_files, plat_bam_plan** plan)
{
    return bamFilesPlanEntry<plat_bam_plan_impl>("plat_bam_files_plan", plan, files, n_files, nullptr, 0, true, [&](plat_bam_plan_impl& I) { return makeBamPlan(files, n_files, I); });
}
CALLER_EXPORT void plat_bam_plan_free(plat_bam_plan* plan) { delete static_cast<plat_bam_plan_impl*>(plan); }

CALLER_EXPORT int plat_bam_files_fetch_plan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions, plat_bam_fetch_plan** plan)
{
    return bamFilesPlanEntry<plat_bam_fetch_plan_impl>("plat_bam_files_fetch_plan", plan, files, n_files, regions, n_regions, true,
                                                       [&](plat_bam_fetch_plan_impl& I) { return makeBamFetchPlan(files, n_files, regions, n_regions, I); });
}
CALLER_EXPORT void plat_bam_fetch_plan_free(plat_bam_fetch_plan* plan) { delete static_cast<plat_bam_fetch_plan_impl*>(plan); }

namespace plathost {

// plat_call_bam_files and plat_call_bam_files_mates (bam_mates.hpp): the plan, the fetch plan, one tid per region, then the BGZF call on
// those structures.  mates(P, X, &units): PLAT_OK with units NULL (no broken mates) or the [n_regions * n_files] units of a mates plan
// (their second round's compressed bytes in *mateBytes), made once the fetch plan stands.
template <class Mates>
inline int callBamFilesWith(plat_caller* c, const char* entry, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                            plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                            plat_fetched_region_info* info, plat_caller_stats* stats, Mates&& mates)
{
    plat_bam_plan_impl P;
    plat_bam_fetch_plan_impl X;
    int rc = guardedEntry(c, entry, [&] {
        const int r = makeBamPlan(files, n_files, P);
        return r != PLAT_OK ? r : makeBamFetchPlan(files, n_files, regions, n_regions, X);
    });
    if (rc != PLAT_OK) return rc;
    // one tid per region: the files that hold the contig have to agree on it
    std::vector<int32_t> tid((size_t)n_regions, 0);
    for (int k = 0; k < n_regions; ++k) {
        int first = -1;
        for (int f = 0; f < n_files; ++f) {
            const plat_bam_fetch& ft = X.F[(size_t)k * n_files + f];
            if (ft.tid < 0) continue;
            if (first < 0) { first = f; tid[(size_t)k] = ft.tid; }
            else if (ft.tid != tid[(size_t)k]) {
                c->lastError = std::string(entry) + ": region " + std::to_string(k) + " (" + regions[k].chrom + "): file " + std::to_string(first) + " has the contig as tid " +
                               std::to_string(tid[(size_t)k]) + ", file " + std::to_string(f) + " as tid " + std::to_string(ft.tid) + "; one call takes one tid per region";
                return PLAT_ERR_UNSUPPORTED;
            }
        }
    }
    const plat_bam_mates* M = nullptr;
    long long mateBytes = 0;
    if ((rc = mates(P, X, &M, &mateBytes)) != PLAT_OK) return rc;
    // the BGZF call's structures (R: plat_bgzf_region or plat_bgzf_rg_region, the units its samples or files): n units per region under the
    // region's head, unit i the fetch of file fileOf(i) with that file's broken mates
    auto fill = [&](auto& units, auto& R, auto unitsOf, int n, auto fileOf, auto setMates) {
        units.resize((size_t)n_regions * (size_t)n); R.resize((size_t)n_regions);
        for (int k = 0; k < n_regions; ++k) {
            for (int i = 0; i < n; ++i) {
                const size_t at = (size_t)k * n_files + fileOf(i);
                auto& u = units[(size_t)k * n + i];
                memset(&u, 0, sizeof u);
                u.n_chunks = X.F[at].n_chunks; u.chunks = X.F[at].chunks;
                if (M) setMates(u, M[at].mates);
            }
            auto& r = R[(size_t)k];
            memset(&r, 0, sizeof r);
            r.chrom = regions[k].chrom; r.start = regions[k].start; r.end = regions[k].end; r.contig_seq = regions[k].contig_seq; r.contig_len = regions[k].contig_len;
            r.dev_contig_seq = regions[k].dev_contig_seq; r.tid = tid[(size_t)k]; r.itr_beg = X.F[(size_t)k * n_files].itr_beg; r.itr_end = X.F[(size_t)k * n_files].itr_end;
            r.*unitsOf = units.data() + (size_t)k * n;
        }
    };
    if (P.mode == PLAT_BAM_FILES_PRESPLIT) {
        std::vector<plat_bgzf_sample> units;
        std::vector<plat_bgzf_region> R;
        fill(units, R, &plat_bgzf_region::samples, P.n_samples, [&](int s) { return P.sample_file[s]; },
             [](plat_bgzf_sample& u, const plat_bam_file_records& m) { u.broken_mates = m.records; });
        rc = plat_call_bgzf_regions(c, R.data(), n_regions, P.n_samples, P.sample_names, options, qc, out_text, out_len, info, stats);
    } else {
        std::vector<plat_bgzf_file> units;
        std::vector<plat_bgzf_rg_region> R;
        fill(units, R, &plat_bgzf_rg_region::files, n_files, [](int f) { return f; }, [](plat_bgzf_file& u, const plat_bam_file_records& m) { u.broken_mates = m; });
        rc = plat_call_bgzf_regions_rg(c, R.data(), n_regions, n_files, &P.groups, P.n_samples, P.sample_names, options, qc, out_text, out_len, info, stats);
    }
    if (rc == PLAT_OK && stats) stats->input_bytes += mateBytes;
    return rc;
}

}  // namespace plathost

CALLER_EXPORT int plat_call_bam_files(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                                      plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                      plat_fetched_region_info* info, plat_caller_stats* stats)
{
    if (!bamFilesCallArgsOk(c, files, n_files, regions, n_regions, options, out_text, out_len)) return PLAT_ERR_INVALID;
    SourceLinesGuard sourceGuard(c);                                       // (whichever way this call ends; the BGZF call behind it holds its own)
    if (options->assemble && options->assembleBrokenPairs) {
        c->lastError = "plat_call_bam_files: assemble=1 with assembleBrokenPairs=1 asks for the mates of improper pairs, a second round of fetches this entry point does not make "
                       "(plat_call_bam_files_mates makes it)";
        return PLAT_ERR_UNSUPPORTED;
    }
    return callBamFilesWith(c, "plat_call_bam_files", files, n_files, regions, n_regions, options, qc, out_text, out_len, info, stats,
                            [](const plat_bam_plan_impl&, const plat_bam_fetch_plan_impl&, const plat_bam_mates**, long long*) { return (int)PLAT_OK; });
}
