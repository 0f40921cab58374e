// bam_rec.hpp -- what the BAM paths share (bam.hip: records -> ranges, bam_reads.hip: records -> reads, bam_write.hip:
// reads -> records): SEQ's alphabet in both directions, the unaligned field readers, the layout predicate every record
// has to pass, and the locator (implemented in bam.hip).
#pragma once

#include "common.hpp"

namespace sarlacc {

constexpr int BAM_TILE = 16384;                  // 64 KB of LDS: two workgroups per CU

// SEQ's alphabet, code -> letter, and its two register tables (each byte-indexed by v_perm_b32, lowest byte first):
// BAM_LETTERS<k> holds the letters of the codes 4 k .. 4 k + 3 (bam_reads.hip), BAM_CODES<k> the codes of the letters
// whose low five bits are 4 k .. 4 k + 3, 0 where there is none (bam_write.hip; the 15 letters are distinct in those bits
// and '=' is never written).
constexpr char BAM_ALPHABET[] = "=ACMGRSVTWYHKDBN";
constexpr uint32_t bam_letters_word(int k) {
    return static_cast<uint32_t>(BAM_ALPHABET[4 * k]) | (static_cast<uint32_t>(BAM_ALPHABET[4 * k + 1]) << 8) |
           (static_cast<uint32_t>(BAM_ALPHABET[4 * k + 2]) << 16) | (static_cast<uint32_t>(BAM_ALPHABET[4 * k + 3]) << 24);
}
constexpr uint32_t bam_code_of(int low5) {
    for (int c = 1; c < 16; ++c)
        if ((BAM_ALPHABET[c] & 31) == low5) return static_cast<uint32_t>(c);
    return 0;
}
constexpr uint32_t bam_codes_word(int k) {
    return bam_code_of(4 * k) | (bam_code_of(4 * k + 1) << 8) | (bam_code_of(4 * k + 2) << 16) | (bam_code_of(4 * k + 3) << 24);
}
constexpr uint32_t BAM_LETTERS0 = bam_letters_word(0), BAM_LETTERS1 = bam_letters_word(1), BAM_LETTERS2 = bam_letters_word(2),
                   BAM_LETTERS3 = bam_letters_word(3);
constexpr uint32_t BAM_CODES0 = bam_codes_word(0), BAM_CODES1 = bam_codes_word(1), BAM_CODES2 = bam_codes_word(2),
                   BAM_CODES3 = bam_codes_word(3), BAM_CODES4 = bam_codes_word(4), BAM_CODES5 = bam_codes_word(5),
                   BAM_CODES6 = bam_codes_word(6), BAM_CODES7 = bam_codes_word(7);
static_assert(BAM_LETTERS0 == 0x4d43413du && BAM_LETTERS3 == 0x4e42444bu, "BAM_LETTERS: lowest byte first");

__device__ __forceinline__ unsigned rd_u32(const uint8_t* p) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);      // records have no alignment
    return v;
}
__device__ __forceinline__ unsigned rd_u16(const uint8_t* p) { return p[0] | (static_cast<unsigned>(p[1]) << 8); }

// The fixed fields both paths read of the record whose block_size field lies at `rec`.
struct BamFixed {
    long long bs, l_name, n_cig, l_seq;
    unsigned flag;
};

// Whether the fields of a located record (block_size >= 32, wholly in the buffer) fit its block size: a name with its
// NUL, l_seq >= 0, and name + CIGAR + SEQ + QUAL inside block_size.  "record fields do not fit its block size" otherwise.
__device__ __forceinline__ bool bam_layout_ok(const uint8_t* rec, BamFixed* F) {
    const uint8_t* f = rec + 4;
    F->bs = static_cast<int>(rd_u32(rec));
    F->l_name = f[8];
    F->n_cig = rd_u16(f + 12);
    F->flag = rd_u16(f + 14);
    F->l_seq = static_cast<int>(rd_u32(f + 16));
    const long long fixed = 32 + F->l_name + 4 * F->n_cig;
    return !(F->l_name == 0 || F->l_seq < 0 || fixed + (F->l_seq + 1) / 2 + F->l_seq > F->bs || f[32 + F->l_name - 1] != 0);
}

// how the chain of records ends in a buffer
enum { BAM_CHAIN_CLEAN = 0, BAM_CHAIN_INCOMPLETE = 1, BAM_CHAIN_SIZE = 2 };

// What the locator found in a buffer: the offsets of the nrec records that lie wholly in it (d_off, nrec + 1 entries of
// the workspace "bam.off", the last one unset), the offset of the first record that does not (nbytes when none is cut)
// and how the chain ends there.  `generation` counts the locator runs of this thread: d_off belongs to the last one.
struct BamLocated {
    long long nrec = 0, end = 0;
    int how = BAM_CHAIN_CLEAN;
    long long* d_off = nullptr;
    unsigned long long generation = 0;
};

// k_bam_hops / k_bam_chain / k_bam_starts over nbytes > 0 of inflated BAM whose byte 0 starts a record, under the stage
// timers bam_hops, bam_chain and bam_starts.  The counts are back on the host when it returns; the launch that writes
// d_off is still on the stream.
int bam_locate(const uint8_t* d_bam, long long nbytes, hipStream_t s, BamLocated* out);
unsigned long long bam_locate_generation();
// The locator's two refusals, for a caller that found no bad record in front of the chain's end (0: none applies).
int bam_chain_end_error(const BamLocated& L, long long first_record, int at_eof);

}  // namespace sarlacc
