// readers.hpp -- what the four readers share: FASTQ text -> reads (fastq.hip), SAM text -> ranges (sam.hip), BAM ->
// ranges (bam.hip) and BAM -> reads (bam_reads.hip).  The module is split like the align, MSA, consensus and UMI stages:
//   readers_host.cpp  everything that decides: the fourteen C entry points, every error text, every workspace, memset,
//                     read-back and stage timer, the line index (line_counts / line_starts), the record back end
//                     (FirstBad, offsets_of, ranges_index), the SAM name table, the BAM locator's launch sequence
//                     (bam_locate) and the state each index call leaves for its extract steps
//   text_lines.hip    kernels and device steps of the line index (text_lines.hpp)
//   fastq.hip, sam.hip, bam.hip, bam_reads.hip   kernels and device steps of one format each
// A kernel is launched only from the file that defines it.  A device step enqueues one launch, or one fixed group of
// launches, on the stream: pointers and sizes in, nothing decided, only HIP errors raised.
//
// A bad input is reported the same way by all four: the fields / size kernel of a format does atomicMin on
// (record << shift | code) into one slot, and the host turns the lowest one into the format's message for that code.
// The codes of a format are listed here in the order its checks run; readers_host.cpp holds one message per code.
#pragma once

#include "common.hpp"

namespace sarlacc {

// ---- FASTQ (fastq.hip) -------------------------------------------------------------------------------------------------------
struct FqRec {
    long long seq_pos, qual_pos, name_pos;
};
constexpr int FQ_BAD_SHIFT = 3;
enum { FQ_BAD_HEADER = 1, FQ_BAD_PLUS = 2, FQ_BAD_LENGTH = 3 };

int fq_records(const uint8_t* text, const long long* line_start, long long nrec, FqRec* rec, long long* seq_len,
               long long* name_len, unsigned long long* first_bad, hipStream_t s);
int fq_copy(const uint8_t* text, const FqRec* rec, const int64_t* off, const int64_t* name_off, long long nrec, uint8_t* seq,
            uint8_t* qual, uint8_t* names, hipStream_t s);

// ---- ranges: SAM lines (sam.hip) and BAM records (bam.hip) ----------------------------------------------------------------------
// per line / record; written for kept ones only
struct SamRec {
    long long name_pos;
    int ref, start, width, lclip, rclip, strand;
};
constexpr int REC_BAD_SHIFT = 4;      // of k_sam_fields, k_bam_fields and k_bamr_size

enum {
    SAM_FIELDS = 1,        // non-blank line with fewer than 6 tab-separated fields
    SAM_FLAG = 2,          // FLAG not an optionally signed decimal int32
    SAM_MAPQ = 3,          // MAPQ likewise
    SAM_POS = 4,           // kept line: POS likewise
    SAM_RNAME = 5,         // kept line: RNAME neither an @SQ name nor '*'
    SAM_CIGAR_STAR = 6,    // kept line: CIGAR '*'
    SAM_CIGAR_SYNTAX = 7,  // kept line: CIGAR not ([0-9]+[MIDNSHP=X])+
    SAM_CIGAR_RANGE = 8,   // kept line: an op length, the width or a clip above 2^31 - 1
    SAM_CIGAR_CLIPS = 9,   // kept line: only H / S ops (the reference's right clip is NA)
    SAM_END = 10,          // kept line: start + width - 1 outside the int32 range
};

// one slot of the open-addressing table of reference names (len < 0: empty)
struct SamName {
    unsigned long long hash;
    long long off;      // into the name bytes
    int len;
    int code;           // seqinfo index, -1 for a `restricted` name that is not in the header
    int restricted;     // listed in `restricted`
    int pad;
};

__host__ __device__ __forceinline__ unsigned long long fnv1a64(const uint8_t* s, long long n) {
    unsigned long long h = 14695981039346656037ull;
    for (long long i = 0; i < n; ++i) {
        h ^= s[i];
        h *= 1099511628211ull;
    }
    return h;
}

int sam_fields(const uint8_t* text, const long long* line_start, long long nlines, const SamName* table, unsigned long long tmask,
               const uint8_t* names, int use_restricted, int use_minq, long long minq, SamRec* rec, int* keep,
               long long* name_len, unsigned long long* first_bad, hipStream_t s);
// the extract step of both formats: `text` is the SAM body or the inflated BAM that SamRec::name_pos points into
int sam_scatter(const uint8_t* text, const SamRec* rec, const int* keep, const int64_t* koff, const int64_t* noff, long long nlines,
                int32_t* ref, int32_t* start, int32_t* width, uint8_t* strand, int32_t* lclip, int32_t* rclip, uint8_t* names,
                int64_t* name_off, hipStream_t s);

enum {
    BAM_LAYOUT = 1,
    BAM_POS = 2,
    BAM_RNAME = 3,
    BAM_CIGAR_STAR = 4,
    BAM_CIGAR_OP = 5,
    BAM_TAGS = 6,
    BAM_CIGAR_RANGE = 7,
    BAM_CIGAR_CLIPS = 8,
    BAM_END = 9,
};

int bam_fields(const uint8_t* bam, const long long* rec_off, long long nrec, long long n_ref, const uint8_t* mask, int use_minq,
               long long minq, SamRec* rec, int* keep, long long* name_len, unsigned long long* first_bad, hipStream_t s);

// ---- the BAM locator (kernels in bam.hip, launch sequence bam_locate in readers_host.cpp) ---------------------------------------
// how the chain of records ends in a buffer
enum { BAM_CHAIN_CLEAN = 0, BAM_CHAIN_INCOMPLETE = 1, BAM_CHAIN_SIZE = 2 };

int bam_hops(const uint8_t* bam, long long nbytes, long long ntiles, unsigned* table, hipStream_t s);
int bam_chain(const unsigned* table, long long nbytes, long long ntiles, long long* entry, hipStream_t s);
// count[tile] = complete records that start in the tile; term = (offset of the first record that is not wholly in the
// buffer, BAM_CHAIN_*), written by the tile in which the chain ends
int bam_starts_count(const uint8_t* bam, long long nbytes, long long ntiles, const long long* entry, long long* count,
                     long long* term, hipStream_t s);
// rec_off = the offsets of those records; base is the exclusive scan of count
int bam_starts_write(const uint8_t* bam, long long nbytes, long long ntiles, const long long* entry, const long long* base,
                     long long* rec_off, hipStream_t s);

// ---- BAM reads (bam_reads.hip) -------------------------------------------------------------------------------------------------
enum { BAMR_LAYOUT = 1, BAMR_SEQ = 2, BAMR_QUAL = 3 };

int bamr_size(const uint8_t* bam, const long long* rec_off, long long nrec, unsigned exclude, int* keep, long long* bases,
              long long* name_len, unsigned long long* first_bad, hipStream_t s);
int bamr_reads(const int* keep, const int64_t* read_of, long long nrec, long long* read_rec, hipStream_t s);
// what the range / extract steps read of an indexed buffer, and the reads first .. first + count in the records a .. e
struct BamrArrays {
    const uint8_t* bam;
    const long long* rec_off;
    const int64_t* base_off;
    const int64_t* name_off;
    const long long* read_rec;
    const int64_t* aux_off;
};
struct BamrRange {
    long long first, count, a, e;
    int64_t bases, name_bytes;
};
// offsets, then SEQ / QUAL where the range has bases, then the names where they are wanted and there are any
int bamr_unpack(const BamrArrays& X, const BamrRange& R, int missing_qual, uint8_t* seq, uint8_t* qual, int64_t* off,
                uint8_t* names, int64_t* name_off, hipStream_t s);
int bamr_aux_len(const uint8_t* bam, const long long* rec_off, const int* keep, long long nrec, long long* aux_len, hipStream_t s);
int bamr_aux(const BamrArrays& X, const BamrRange& R, uint8_t* aux, int64_t* aux_off, hipStream_t s);

}  // namespace sarlacc
