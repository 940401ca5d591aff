// bam_aux.hpp -- every part of plat_bamroute.hip that indexes memory from input bytes, as plain functions that compile for the host too:
// where a record's aux area starts (from its fixed fields), the bounded walk over the aux fields to the first RG field, the extent and
// the hash of its value, and the look-up of that value in the read-group table (hash probe, then a comparison of the bytes).
//
// A restatement of the reference loader's rule (ReadIterator.get(1, &rgID), htslibWrapper.pyx:348-361: bam_aux_get(b, "RG") and
// bam_aux2Z; samplesByID[rgID], platypusutils.pyx:573-666) over the aux layout of the SAM/BAM specification section 4.2.4; the rule is
// written out at plat_bam_route_batch (include/platypus_mi355x.h).
//
// The record is the half-open byte range [off, end) of whatever `Bytes` indexes.  Every read is of an index i with off <= i < end: the
// walk keeps a cursor `at` with off <= at <= end and reads at + k only after checking k < end - at.  Every loop either moves the cursor
// forward by at least 3 bytes or runs over a range checked to lie inside the record, so no input makes it spin.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BAMAUX_HD __host__ __device__ inline
#else
#define BAMAUX_HD inline
#endif

namespace bamaux {

// verdicts: ROUTED, or why the record is refused (the values of plat_bam_route_out.why)
constexpr int ROUTED = 0;
constexpr int NO_RG = 1;                                  // the walk ended without an RG field
constexpr int RG_NOT_STRING = 2;                          // the first RG field has a type other than Z or H
constexpr int NOT_IN_TABLE = 3;                           // its value is no ID of the table
constexpr int UNKNOWN_TYPE = 4;                           // a field's type, or a B field's subtype, is none of the specification's
constexpr int NEGATIVE_COUNT = 5;                         // a B field's count is negative
constexpr int AUX_OVERRUN = 6;                            // a field, a string's NUL or an array runs past the record's end
constexpr int FIXED_OVERRUN = 7;                          // the fixed part (32 bytes, name, CIGAR, bases, qualities) runs past the record's end

constexpr uint32_t HASH_SEED = 2166136261u, HASH_PRIME = 16777619u;               // FNV-1a, 32 bits
BAMAUX_HD uint32_t hash_step(uint32_t h, uint8_t b) { return (h ^ b) * HASH_PRIME; }

template <class Bytes> BAMAUX_HD uint32_t ld16(const Bytes& m, int64_t at) { return (uint32_t)m[at] | ((uint32_t)m[at + 1] << 8); }
template <class Bytes> BAMAUX_HD uint32_t ld32(const Bytes& m, int64_t at) { return ld16(m, at) | (ld16(m, at + 2) << 16); }

// bytes of one value of a fixed-size type (0: not such a type)
BAMAUX_HD int fixed_size(uint8_t type) {
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'd': return 8;
    default: return 0;
    }
}
// ... of one element of a B array (0: no subtype of the specification; d is none)
BAMAUX_HD int array_elem_size(uint8_t sub) { return sub == 'd' || sub == 'A' ? 0 : fixed_size(sub); }

// The offset of the aux area inside [off, end), or -1 when the fixed part does not fit (l_seq is read as the unsigned word the
// specification gives it: a negative one does not fit).  Reads off .. off + 19 only after end - off >= 32.
template <class Bytes> BAMAUX_HD int64_t aux_start(const Bytes& m, int64_t off, int64_t end)
{
    if (off < 0 || end - off < 32) return -1;
    const int64_t lName = m[off + 8], nCig = ld16(m, off + 12), lSeq = ld32(m, off + 16);
    const int64_t at = 32 + lName + 4 * nCig + (lSeq + 1) / 2 + lSeq;                 // (< 2^34: no overflow)
    return at > end - off ? -1 : off + at;
}

// The walk: the first RG field's value as [*val, *val + *val_len) (without its NUL) and its hash.  Returns ROUTED (found; the look-up
// is still to come) or the refusal.
template <class Bytes> BAMAUX_HD int find_rg(const Bytes& m, int64_t off, int64_t end, int64_t* val, int64_t* val_len, uint32_t* hash)
{
    int64_t at = aux_start(m, off, end);
    if (at < 0) return FIXED_OVERRUN;
    while (end - at >= 3) {                                                        // (every round moves `at` forward by >= 3, or returns)
        const uint8_t t0 = m[at], t1 = m[at + 1], type = m[at + 2];
        at += 3;
        if (t0 == 'R' && t1 == 'G') {
            if (type != 'Z' && type != 'H') return RG_NOT_STRING;
            uint32_t h = HASH_SEED;
            for (int64_t k = at; k < end; ++k) {
                const uint8_t b = m[k];
                if (b == 0) { *val = at; *val_len = k - at; *hash = h; return ROUTED; }
                h = hash_step(h, b);
            }
            return AUX_OVERRUN;
        }
        if (type == 'Z' || type == 'H') {
            int64_t k = at;
            while (k < end && m[k] != 0) ++k;
            if (k >= end) return AUX_OVERRUN;
            at = k + 1;
        } else if (type == 'B') {
            if (end - at < 5) return AUX_OVERRUN;
            const int64_t size = array_elem_size(m[at]), count = (int32_t)ld32(m, at + 1);
            if (size == 0) return UNKNOWN_TYPE;
            if (count < 0) return NEGATIVE_COUNT;
            if (count * size > end - at - 5) return AUX_OVERRUN;                   // (count * size < 2^33)
            at += 5 + count * size;
        } else {
            const int64_t size = fixed_size(type);
            if (size == 0) return UNKNOWN_TYPE;
            if (size > end - at) return AUX_OVERRUN;
            at += size;
        }
    }
    return NO_RG;
}

// ---- the read-group table -------------------------------------------------------------------------------------------------------
// n_groups IDs, their bytes back to back (ID g = ids[id_off[g] .. id_off[g + 1])), and an open-addressed table of `mask + 1` slots
// (a power of two >= 2 * n_groups, so a probe always meets an empty slot): slot_group[s] < 0 = empty, else the group whose ID hashes to
// slot_hash[s].  Equal IDs each take a slot; the look-up returns the lowest group among them.
struct GroupTable {
    const uint32_t* slot_hash;
    const int32_t* slot_group;
    uint32_t mask;
    const uint8_t* ids;
    const int32_t* id_off;
};

BAMAUX_HD uint32_t table_slots(int32_t n_groups) {
    uint32_t p = 2;
    while (p < 2u * (uint32_t)n_groups) p <<= 1;
    return p;
}

BAMAUX_HD uint32_t hash_id(const uint8_t* id, int32_t len) {
    uint32_t h = HASH_SEED;
    for (int32_t k = 0; k < len; ++k) h = hash_step(h, id[k]);
    return h;
}

// the serial build (host; the device builds the same table with an atomic compare-and-swap per slot)
inline void table_insert(uint32_t* slot_hash, int32_t* slot_group, uint32_t mask, uint32_t h, int32_t g) {
    uint32_t s = h & mask;
    while (slot_group[s] >= 0) s = (s + 1) & mask;
    slot_group[s] = g; slot_hash[s] = h;
}

// the value [val, val + len) of the record against ID g, byte by byte
template <class Bytes> BAMAUX_HD bool id_equal(const Bytes& m, int64_t val, int64_t len, const GroupTable& t, int32_t g) {
    const int32_t a = t.id_off[g];
    if ((int64_t)t.id_off[g + 1] - a != len) return false;
    for (int64_t k = 0; k < len; ++k) if (m[val + k] != t.ids[a + k]) return false;
    return true;
}

// the group of the value, or -1: a slot whose hash matches is a candidate only; the bytes decide
template <class Bytes> BAMAUX_HD int32_t lookup(const Bytes& m, int64_t val, int64_t len, uint32_t h, const GroupTable& t) {
    int32_t best = -1;
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {                           // (at most one round over the table)
        const uint32_t s = (h + probe) & t.mask;
        const int32_t g = t.slot_group[s];
        if (g < 0) break;
        if (t.slot_hash[s] == h && (best < 0 || g < best) && id_equal(m, val, len, t, g)) best = g;
    }
    return best;
}

// the whole rule for one record: *group is the table's group (its sample: group_sample[*group]) when ROUTED
template <class Bytes> BAMAUX_HD int route(const Bytes& m, int64_t off, int64_t end, const GroupTable& t, int32_t* group) {
    int64_t val = 0, len = 0;
    uint32_t h = 0;
    *group = -1;
    const int v = find_rg(m, off, end, &val, &len, &h);
    if (v != ROUTED) return v;
    *group = lookup(m, val, len, h, t);
    return *group < 0 ? NOT_IN_TABLE : ROUTED;
}

}  // namespace bamaux
