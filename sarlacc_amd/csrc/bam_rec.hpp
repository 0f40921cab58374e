// bam_rec.hpp -- what the BAM paths share (bam.hip: records -> ranges, bam_reads.hip: records -> reads, bam_write.hip:
// reads -> records, bam_tags.hip: the tags of resident reads): SEQ's alphabet in both directions, the unaligned field
// readers, the layout predicate every record has to pass, and the tag walker.  (The locator's interface is in readers.hpp.)
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

// bytes of a tag value of a fixed-size type, 0 for any other letter
__device__ __forceinline__ int bam_type_size(int t) {
    if (t == 'A' || t == 'c' || t == 'C') return 1;
    if (t == 's' || t == 'S') return 2;
    if (t == 'i' || t == 'I' || t == 'f') return 4;
    return 0;
}

// ---- the tag walker ------------------------------------------------------------------------------------------------------
// An aux area is the bytes behind QUAL up to the record's end (SAM specification section 4.2.4): entries of tag (two
// bytes), type letter, value.  bam_tag_next steps over one entry, the whole wavefront together and every value the
// same in all its lanes.  It never reads at or behind `end`, whatever the bytes say.  Malformed: fewer than 3 bytes in
// front of the end, a type letter outside AcCsSiIfZHB, a fixed value or a B header or payload past the end, a B subtype
// outside cCsSiIf, a Z or H without a NUL in front of the end.
typedef uint32_t __attribute__((ext_vector_type(4))) bam_u32x4;
typedef bam_u32x4 __attribute__((aligned(1))) bam_u32x4_unaligned;

struct BamTag {
    unsigned name = 0;               // the two tag bytes, the first one low
    int type = 0;
    long long at = 0, val = 0, val_len = 0, next = 0;    // entry start, value start, value bytes (Z / H: without the NUL;
                                                         // B: with its 5-byte header), start of the next entry
};

enum { BAM_TAG_OK = 0, BAM_TAG_END = 1, BAM_TAG_BAD = 2 };

// first NUL among aux[p .. end), `end` when there is none: 16 bytes per lane and step, the tail byte by byte
__device__ __forceinline__ long long bam_wave_find_nul(const uint8_t* aux, long long p, long long end, int lane) {
    for (long long q0 = p; q0 < end; q0 += 16 * 64) {
        const long long q = q0 + 16LL * lane;
        int hit = -1;
        if (q + 16 <= end) {
            const bam_u32x4 v = *reinterpret_cast<const bam_u32x4_unaligned*>(aux + q);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                const uint32_t z = (w[i] - 0x01010101u) & ~w[i] & 0x80808080u;     // its lowest set bit: the first NUL of the word
                if (z) hit = 4 * i + ((__ffs(static_cast<int>(z)) - 1) >> 3);
            }
        } else {
            for (long long j = end - 1; j >= q; --j)
                if (aux[j] == 0) hit = static_cast<int>(j - q);
        }
        const unsigned long long any = __ballot(hit >= 0);
        if (any) {
            const int first = __ffsll(static_cast<long long>(any)) - 1;
            return q0 + 16LL * first + __shfl(hit, first);
        }
    }
    return end;
}

// the entry at aux[p], p <= end
__device__ __forceinline__ int bam_tag_next(const uint8_t* aux, long long p, long long end, int lane, BamTag* T) {
    if (p >= end) return BAM_TAG_END;
    if (end - p < 3) return BAM_TAG_BAD;
    T->at = p;
    T->name = aux[p] | (static_cast<unsigned>(aux[p + 1]) << 8);
    const int ty = aux[p + 2];
    T->type = ty;
    T->val = p + 3;
    long long sz = bam_type_size(ty);
    if (sz) {
        T->val_len = sz;
    } else if (ty == 'Z' || ty == 'H') {
        const long long nul = bam_wave_find_nul(aux, p + 3, end, lane);
        if (nul >= end) return BAM_TAG_BAD;
        T->val_len = nul - (p + 3);
        sz = T->val_len + 1;
    } else if (ty == 'B') {
        if (end - (p + 3) < 5) return BAM_TAG_BAD;
        const int es = aux[p + 3] == 'A' ? 0 : bam_type_size(aux[p + 3]);
        if (!es) return BAM_TAG_BAD;
        sz = 5 + static_cast<long long>(rd_u32(aux + p + 4)) * es;
        T->val_len = sz;
    } else {
        return BAM_TAG_BAD;
    }
    if (sz > end - (p + 3)) return BAM_TAG_BAD;
    T->next = p + 3 + sz;
    return BAM_TAG_OK;
}

}  // namespace sarlacc
