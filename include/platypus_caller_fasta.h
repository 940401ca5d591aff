/*
 * platypus_caller_fasta.h -- the reference FASTA for the native region loop (libplat_caller.so): the file's bytes and its .fai taken as
 * they lie on disk, contigs and sequence windows fetched on the device.
 *
 * plat_region.contig_seq / dev_contig_seq (include/platypus_caller.h; the fetched, BAM, BGZF and read-group regions have the same two
 * fields) want a contig in memory: upper case, no newlines.  FastaFile (src/cython/fastafile.pyx) makes that of the file with line
 * arithmetic on the index, replace("\n", "") and upper().  Here the library does it, on the device (plat_fasta_fetch_batch,
 * include/platypus_mi355x.h states the rule; csrc/fasta_rule.hpp is the rule as code and the host twin):
 *
 *   plat_fasta_open        the file's bytes (they may be a mapped file; they must stay valid until plat_fasta_close) and the .fai's bytes.
 *                          The index is parsed HERE, on the host -- it is serial and a few KB -- by FastaIndex.getRefs' rule (:64-82): per
 *                          line strip(), split on tabs, the name the first white-space-separated token of field 0 (with parseNCBI a name
 *                          gi|..|ref|X|.. becomes X), fields 1 to 4 through atoll; a later line with the same name replaces the earlier
 *                          one's numbers and keeps its place.  Nothing is uploaded yet
 *   plat_fasta_load        the contigs tids[0 .. n) (n == 0: all of them): the part of the file from the first of their spans to the end
 *                          of the last is uploaded, ONE device batch in whole-contig mode runs on the caller's first stream, one wait,
 *                          one copy back into pinned host memory the object owns (plat_region.contig_seq must be host memory)
 *   plat_fasta_contig      the two pointers an integrator puts into plat_region.contig_seq and .dev_contig_seq, and contig_len: all
 *                          SeqLength bases as the file holds them (fewer where the file ends early).  Loads the contig when it is not
 *                          loaded.  Both are followed by PLAT_BLOB_PAD zero bytes and stay valid until plat_fasta_close
 *   plat_fasta_get_sequences   getSequence(name, beg, end) for a batch, answered from the file's bytes: the part of the file that holds
 *                          the queries' spans is uploaded, one device batch, one wait.  status[q] is PLAT_FASTA_OK, PLAT_FASTA_INDEX_ERROR (the
 *                          reference's IndexError: end < beg after the clamps) or PLAT_FASTA_ZERO_LINE; the bytes of q are
 *                          bytes[first[q] .. first[q + 1])
 *   plat_fasta_get_character   getCharacter(name, pos) (:120-139), on the host: one byte of the file
 *
 * A FASTA object belongs to the caller it was opened on: it uses that caller's first stream, must be closed before the caller is
 * destroyed and -- like every entry point of a caller -- is used by one thread at a time.  What plat_fasta_get_sequences returns is owned
 * by the object until its next call or its close.
 *
 * Refused at open with a message in plat_caller_last_error that names the line (from 1), the caller staying usable
 * (PLAT_ERR_BAD_INPUT): a line with fewer than five tab-separated fields or without a name token -- the reference raises there; a blank
 * line is one --; and, as stated limits where the reference would seek to a negative offset: StartPos < 0, LineLength < 0,
 * SeqLength < 0, FullLineLength < LineLength.  A line with LineLength 0 opens: the reference divides by it only when the contig is asked
 * for, so plat_fasta_get_sequences gives such a query PLAT_FASTA_ZERO_LINE, and plat_fasta_load, plat_fasta_contig and
 * plat_fasta_get_character refuse the contig (PLAT_ERR_BAD_INPUT, naming it).  A tid outside the index is PLAT_ERR_INVALID, naming it.  A library
 * linked against a device library without plat_fasta_fetch_batch returns PLAT_ERR_UNSUPPORTED from plat_fasta_load, plat_fasta_contig
 * and plat_fasta_get_sequences, naming the symbol; PLAT_CALLER_HOST_FASTA=1 answers all three with the host twin instead (tests,
 * measurements; read once per call with the other switches; dev_seq is then NULL).
 * Not handled: reading files from disk, writing a .fai, bgzipped FASTA with a .gzi.
 */
#ifndef PLATYPUS_CALLER_FASTA_H
#define PLATYPUS_CALLER_FASTA_H

#include "platypus_caller.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plat_fasta plat_fasta;

int plat_fasta_open(plat_caller* c, const uint8_t* file_bytes, int64_t file_len, const uint8_t* fai_bytes, int64_t fai_len, int parseNCBI, plat_fasta** out);
int plat_fasta_close(plat_fasta* ref);
int plat_fasta_n_refs(const plat_fasta* ref);
/* Contig i in file order: its name (NUL-ended, the object's memory) and SeqLength.  PLAT_ERR_INVALID outside the index. */
int plat_fasta_ref(const plat_fasta* ref, int i, const char** name, int64_t* seq_len);
/* ... and the other three numbers of its line. */
int plat_fasta_ref_line(const plat_fasta* ref, int i, int64_t* start_pos, int64_t* line_len, int64_t* full_line_len);
/* The tid of a name, -1 when absent; names compare byte by byte over their whole length. */
int plat_fasta_tid(const plat_fasta* ref, const char* name);
/* getTotalSequenceLength: the sum of SeqLength over the index. */
int64_t plat_fasta_total_length(const plat_fasta* ref);

typedef struct plat_fasta_info {
    int64_t queries;                 /* contigs or queries of the call */
    int64_t file_bytes;              /* bytes of the file that were uploaded (0 on the host path) */
    int64_t out_bytes;               /* bytes of all answers */
    int64_t device_calls;            /* 0 on the host path */
    double seconds;                  /* the whole call */
} plat_fasta_info;

int plat_fasta_load(plat_fasta* ref, const int32_t* tids, int n /* 0: all */, plat_fasta_info* info /* may be NULL */);
int plat_fasta_contig(plat_fasta* ref, int tid, const uint8_t** host_seq, const uint8_t** dev_seq, int64_t* len);
int plat_fasta_get_sequences(plat_fasta* ref, int n, const int32_t* tid, const int64_t* beg, const int64_t* end,
                             const int64_t** first, const uint8_t** bytes, const int32_t** status, plat_fasta_info* info /* may be NULL */);
/* *n_out: 1, or 0 where the file ends in front of the base's offset (the reference's read returns an empty string there). */
int plat_fasta_get_character(const plat_fasta* ref, int tid, int64_t pos, uint8_t* out, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_FASTA_H */
