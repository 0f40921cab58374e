// bam_write.hip -- resident read batch -> unaligned BAM records, on gfx950: the inverse of bam_reads.hip's k_bamr_unpack.
//
// Record i is an unmapped, unpaired alignment record (SAM specification section 4.2), L its bases, l_read_name the
// bytes of its name with the NUL:
//
//     block_size (int32, not counting itself) | refID -1 | pos -1 | l_read_name | mapq 0 | bin 4680 | n_cigar_op 0 |
//     flag 4 | l_seq | next_refID -1 | next_pos -1 | tlen 0 | name NUL | SEQ | QUAL          (36 + l_read_name + (L + 1) / 2 + L bytes)
//
// SEQ holds two 4-bit codes per byte through "=ACMGRSVTWYHKDBN", high nibble first, the low nibble of an odd last byte 0;
// QUAL holds byte - 33; a batch with tags (the raw aux bytes of every read, bam_tags.hip) has each read's aux bytes behind
// QUAL, counted in block_size, and there are no tags otherwise.  The name is the read's name up to its first space or
// tab ('*' where nothing is left), READ_<first_index + i> when the batch has no names.  The stream holds records only: the caller puts the
// header in front and compresses (bgzf_deflate.hip, which takes the SEQ and QUAL starts this file reports as the ends
// of its pieces).
//
//   k_bamw_size    one wavefront per record: the kept part of the name, then name, bases and qualities scanned 16
//                  bytes per lane and step; the byte length of the record
//   (rocPRIM exclusive scan: n + 1 record offsets, the last one is the size of the stream)
//   k_bamw_cuts    SEQ start and QUAL start of every record in the stream, with tags the tag start as well
//   k_bamw_format  the bytes of a contiguous record range, divided by OUTPUT bytes as k_fqw_format is: the walk
//                  out_tiles.hpp describes (this kernel's own copy of it), 16-byte pieces aligned in memory.  A piece
//                  inside SEQ packs 32 bases read with two unaligned 16-byte loads: the letter's low five bits index a
//                  32-entry table of codes held in eight registers (bam_rec.hpp; the 15 letters are distinct in those
//                  bits), read with v_perm_b32 four letters at a time.  A piece inside QUAL is one unaligned 16-byte load.  A piece
//                  that holds fixed fields, a name, the first or last bytes of SEQ or QUAL or a record boundary is
//                  assembled byte by byte in the lane's registers and leaves as one 16-byte store too; only the two
//                  ends of the range are stored byte by byte.
//
// No kernel waits on another workgroup and every loop is bounded by a record's own length or the range.  A batch BAM
// cannot hold is an error return of the size pass (first_bad: atomicMin on record << 20 | tag << 4 | code, on the
// failure path only, as k_bamr_size reports), before a byte is written.
//
// The three kernels are templates on "with tags" (sarlacc_dev_bam_format_size_aux / _format_aux); the instantiations
// without are the kernels as they were.
//
// Messages, "record K: <reason>", K 1-based; the lowest record wins, within a record name, SEQ, QUAL, tags:
//   read name longer than 254 bytes              (after the cut)
//   read name holds a byte outside '!'..'~'      (in the kept part)
//   base cannot be stored in BAM                 (anything but the 15 upper-case letters: '=', lower case, '-')
//   quality byte outside Phred+33                (outside 33..126)
//   malformed tags                               (bam_rec.hpp's walker; in front of a repeat in the same record)
//   tag XX appears twice
//   record larger than 2^31 - 1 bytes
// Out of scope: aligned records, paired flags, qualities written as the 0xff "missing" marker.
#include "bam_rec.hpp"
#include "out_tiles.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <type_traits>

namespace sarlacc {
namespace {

enum { BAMW_NAME_LONG = 1, BAMW_NAME_BYTE = 2, BAMW_BASE = 3, BAMW_QUAL = 4, BAMW_SIZE = 5, BAMW_TAGS = 6, BAMW_TAG_TWICE = 7 };

constexpr int BW_FIXED = 36;                      // block_size and the fixed fields
constexpr int BW_NAME_MAX = 254;                  // l_read_name is a byte and counts the NUL
constexpr uint32_t BW_BIN = 4680;                 // reg2bin(-1, 0)
constexpr uint32_t BW_FLAG = 4;                   // unmapped

// codes of the four letters of w, byte by byte (bam_rec.hpp's table of codes); 0 where the low five bits are those of
// no letter
__device__ __forceinline__ uint32_t codes4(uint32_t w) {
    const uint32_t sel = w & 0x07070707u;
    const uint32_t p0 = __builtin_amdgcn_perm(BAM_CODES1, BAM_CODES0, sel), p1 = __builtin_amdgcn_perm(BAM_CODES3, BAM_CODES2, sel);
    const uint32_t p2 = __builtin_amdgcn_perm(BAM_CODES5, BAM_CODES4, sel), p3 = __builtin_amdgcn_perm(BAM_CODES7, BAM_CODES6, sel);
    const uint32_t m3 = ((w >> 3) & 0x01010101u) * 0xffu, m4 = ((w >> 4) & 0x01010101u) * 0xffu;
    const uint32_t lo = (p1 & m3) | (p0 & ~m3), hi = (p3 & m3) | (p2 & ~m3);
    return (hi & m4) | (lo & ~m4);
}

// non-zero iff one of the four bytes of w is not one of the 15 letters (they lie in 0x41 .. 0x59)
__device__ __forceinline__ uint32_t not_base4(uint32_t w) {
    const uint32_t c = codes4(w);
    return ((w & 0xe0e0e0e0u) ^ 0x40404040u) | ((c - 0x01010101u) & ~c & 0x80808080u);
}

// non-zero iff one of the four bytes of w lies outside 33 .. 126
__device__ __forceinline__ uint32_t not_phred4(uint32_t w) {
    const uint32_t low = w & 0x7f7f7f7fu;
    return (w | ~(low + 0x5f5f5f5fu) | (low + 0x01010101u)) & 0x80808080u;
}

// two SEQ bytes of the four codes of c: the first code in the high nibble
__device__ __forceinline__ uint32_t pack4(uint32_t c) {
    const uint32_t x = (c << 4) | (c >> 8);
    return (x & 0xffu) | ((x >> 8) & 0xff00u);
}

__device__ __forceinline__ long long wave_min(long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const long long t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}

// *blank: the first space or tab among the n bytes at p; *other: the first other byte outside '!'..'~' (n: none)
__device__ __forceinline__ void wave_name_scan(const uint8_t* p, long long n, int lane, long long* blank, long long* other) {
    long long fb = n, fo = n;
    for (long long q = 16LL * lane; q < n; q += 16 * 64) {
        const long long e = q + 16 < n ? q + 16 : n;
        for (long long j = q; j < e; ++j) {
            const uint8_t c = p[j];
            if (c == ' ' || c == '\t') fb = j < fb ? j : fb;
            else if (c < '!' || c > '~') fo = j < fo ? j : fo;
        }
    }
    *blank = wave_min(fb);
    *other = wave_min(fo);
}

// The tags of a batch (AUX instantiations): the raw aux bytes of every read, flat, with n + 1 offsets.
struct BwAux {
    const uint8_t* aux; const int64_t* aux_off;
};

// Whether the aux area A[0 .. end) can go behind QUAL: 0, BAMW_TAGS for a malformed one, BAMW_TAG_TWICE (*twice: the
// tag of the first such entry) where two entries of a well-formed one carry one tag.  The whole wavefront walks the
// entries (bam_tag_next); the tags of the first 64 entries sit one per lane and a new one is compared with all of them
// in one ballot.  Entries from the 65th on are also compared with the entries 64 .. by a walk of their own each -- no
// basecaller or mapper writes that many.
__device__ __forceinline__ int bamw_aux_check(const uint8_t* A, long long end, int lane, unsigned* twice) {
    BamTag T;
    unsigned mine = 0xffffffffu;      // no tag: a tag is 16 bits
    long long p = 0;
    int st;
    bool found = false;               // a repeat is reported only once the whole area has proved well-formed
    for (long long i = 0; (st = bam_tag_next(A, p, end, lane, &T)) == BAM_TAG_OK; ++i, p = T.next) {
        if (found) continue;
        bool dup = __ballot(mine == T.name) != 0;
        if (!dup && i > 64) {
            BamTag U;
            long long q = 0;
            for (long long j = 0; j < i && !dup; ++j, q = U.next) {      // (entries in front of a well-formed one are well-formed)
                bam_tag_next(A, q, end, lane, &U);
                dup = j >= 64 && U.name == T.name;
            }
        }
        if (dup) { *twice = T.name; found = true; }
        if (lane == i) mine = T.name;
    }
    return st == BAM_TAG_BAD ? BAMW_TAGS : found ? BAMW_TAG_TWICE : 0;
}

// len[r] = bytes of record r, 0 for a refused one (len[n] = 0 for the scan); first_bad: lowest refused record << 20 |
// the tag of BAMW_TAG_TWICE << 4 | why
template <bool AUX>
__global__ void __launch_bounds__(OT_THREADS) k_bamw_size(const uint8_t* seq, const uint8_t* qual, const int64_t* off,
                                                          const uint8_t* names, const int64_t* name_off, long long first_index,
                                                          long long n, BwAux X, long long* len, unsigned long long* first_bad) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = static_cast<long long>(gridDim.x) * (OT_THREADS / 64);
    if (blockIdx.x == 0 && threadIdx.x == 0) len[n] = 0;
    for (long long r = static_cast<long long>(blockIdx.x) * (OT_THREADS / 64) + (threadIdx.x >> 6); r < n; r += nwaves) {
        const long long so = off[r], L = off[r + 1] - so;
        long long l_name;
        int bad = 0;
        if (names) {
            const long long no = name_off[r];
            long long kept, other;
            wave_name_scan(names + no, name_off[r + 1] - no, lane, &kept, &other);
            if (kept > BW_NAME_MAX) bad = BAMW_NAME_LONG;
            else if (other < kept) bad = BAMW_NAME_BYTE;
            l_name = (kept > 0 ? kept : 1) + 1;      // '*' for an empty name
        } else {
            l_name = NAME_PREFIX + decimal_width(static_cast<unsigned long long>(first_index + r)) + 1;
        }
        if (!bad && wave_any_bad(seq + so, L, lane, [](uint32_t w) { return not_base4(w); },
                                 [](uint8_t c) { return not_base4(c | 0x41414100u) != 0; })) bad = BAMW_BASE;
        if (!bad && wave_any_bad(qual + so, L, lane, [](uint32_t w) { return not_phred4(w); },
                                 [](uint8_t c) { return c < 33 || c > 126; })) bad = BAMW_QUAL;
        long long total = BW_FIXED + l_name + (L + 1) / 2 + L;
        unsigned twice = 0;
        if constexpr (AUX) {
            const long long ao = X.aux_off[r], al = X.aux_off[r + 1] - ao;
            if (!bad) bad = bamw_aux_check(X.aux + ao, al, lane, &twice);
            total += al;
        }
        if (!bad && total > 0x7fffffffLL) bad = BAMW_SIZE;
        if (lane == 0) {
            len[r] = bad ? 0 : total;
            if (bad) atomicMin(first_bad, (static_cast<unsigned long long>(r) << 20) | (twice << 4) | static_cast<unsigned>(bad));
        }
    }
}

// cuts[2 r], cuts[2 r + 1] = where SEQ and QUAL of record r start in the stream; with tags cuts[3 r], cuts[3 r + 1] and
// in cuts[3 r + 2] where the tags start (the record's end where it has none)
template <bool AUX>
__global__ void __launch_bounds__(256) k_bamw_cuts(const int64_t* off, const int64_t* rec_off, BwAux X, long long n, int64_t* cuts) {
    const long long r = blockIdx.x * 256LL + threadIdx.x;
    if (r >= n) return;
    const long long al = AUX ? X.aux_off[r + 1] - X.aux_off[r] : 0;
    const long long L = off[r + 1] - off[r], ql = rec_off[r + 1] - al - L;
    constexpr int PER = AUX ? 3 : 2;
    cuts[PER * r] = ql - (L + 1) / 2;
    cuts[PER * r + 1] = ql;
    if (AUX) cuts[PER * r + 2] = ql + L;
}

// what a lane knows about the record it is writing
struct BwRec {
    long long r = -1, start = 0, len = 0;    // record, its first byte in the whole stream, its length
    long long so = 0, sl = 0, no = 0;        // sequence / quality offset and length, name offset
    int l_name = 0;                          // bytes of the name with its NUL
    bool star = false;                       // nothing of the name is kept: '*'
};
struct BwRecAux : BwRec {
    long long ao = 0, al = 0;                // tag offset and length
};

struct BwSource {
    const uint8_t* seq; const uint8_t* qual; const int64_t* off;
    const uint8_t* names; const int64_t* name_off; long long first_index;
    const int64_t* rec_off;

    __device__ __forceinline__ void load(BwRecAux& R, long long r, const BwAux& X) const {
        R.ao = X.aux_off[r];
        R.al = X.aux_off[r + 1] - R.ao;
        load(R, r, R.al);
    }

    __device__ __forceinline__ void load(BwRec& R, long long r, long long al = 0) const {
        R.r = r;
        R.start = rec_off[r];
        R.len = rec_off[r + 1] - R.start;
        R.so = off[r];
        R.sl = off[r + 1] - R.so;
        R.l_name = static_cast<int>(R.len - al - BW_FIXED - (R.sl + 1) / 2 - R.sl);
        R.star = false;
        if (names) {
            R.no = name_off[r];
            // one byte kept: the name's own first byte, or '*' where that is a blank or there is none
            if (R.l_name == 2) R.star = name_off[r + 1] == R.no || names[R.no] == ' ' || names[R.no] == '\t';
        }
    }

    // byte q of record R with tags
    __device__ __forceinline__ uint8_t byte_at(const BwRecAux& R, long long q, const BwAux& X) const {
        const long long body = R.len - R.al;
        return q < body ? byte_at(static_cast<const BwRec&>(R), q) : X.aux[R.ao + (q - body)];
    }

    // byte q of record R (in front of its tags)
    __device__ __forceinline__ uint8_t byte_at(const BwRec& R, long long q) const {
        if (q < BW_FIXED) {
            const int f = static_cast<int>(q >> 2);
            const uint32_t v = f == 0 ? static_cast<uint32_t>(R.len - 4)
                             : f == 3 ? static_cast<uint32_t>(R.l_name) | (BW_BIN << 16)      // l_read_name, mapq 0, bin
                             : f == 4 ? BW_FLAG << 16                                          // n_cigar_op 0, flag
                             : f == 5 ? static_cast<uint32_t>(R.sl)
                             : f == 8 ? 0u : 0xffffffffu;                                      // tlen; refID, pos, next_refID, next_pos
            return static_cast<uint8_t>(v >> (8 * (q & 3)));
        }
        q -= BW_FIXED;
        if (q < R.l_name) {
            if (q == R.l_name - 1) return 0;
            if (!names) return default_name_char(static_cast<unsigned long long>(first_index + R.r), R.l_name - 1, static_cast<int>(q));
            return R.star ? static_cast<uint8_t>('*') : names[R.no + q];
        }
        q -= R.l_name;
        const long long nseq = (R.sl + 1) / 2;
        if (q < nseq) {
            uint32_t c = (codes4(seq[R.so + 2 * q]) & 15u) << 4;
            if (2 * q + 1 < R.sl) c |= codes4(seq[R.so + 2 * q + 1]) & 15u;
            return static_cast<uint8_t>(c);
        }
        return static_cast<uint8_t>(qual[R.so + (q - nseq)] - 33);
    }
};

// out[0 .. ) = bytes rec_off[first] .. rec_off[first + count] of the whole stream.  This kernel keeps its own copy of
// walk_out_tiles and of OutPiece (out_tiles.hpp; change them together): as a body of the shared walk it left its
// occupancy step or ran 2 - 5 % longer on 200-base reads (profiles/io_tile_walk_device_code.txt, io_tile_walk_speed.txt).
// AUX: the tags are one more kind of piece behind QUAL, a whole piece inside them one unaligned 16-byte load, and a
// lane carries their offset and length as well (BwRecAux); the instantiation without them is the kernel as it was.
template <bool AUX>
__global__ void __launch_bounds__(OT_THREADS) k_bamw_format(BwSource S, BwAux X, long long first, long long count, uint8_t* out) {
    constexpr int BW_TILE = 64 * 16 * OT_PIECES;      // bytes of the stream per wavefront and step
    const long long base = S.rec_off[first], nbytes = S.rec_off[first + count] - base;
    const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(out) & 15);   // pieces are aligned in memory, not in the stream
    const long long ntiles = (nbytes + mis + BW_TILE - 1) / BW_TILE;
    const int lane = threadIdx.x & 63;
    const long long wave = blockIdx.x * static_cast<long long>(OT_THREADS / 64) + (threadIdx.x >> 6);
    const long long nwaves = static_cast<long long>(gridDim.x) * (OT_THREADS / 64);
    typename std::conditional<AUX, BwRecAux, BwRec>::type R;
    const auto load = [&](long long r) { if constexpr (AUX) S.load(R, r, X); else S.load(R, r); };
    for (long long tile = wave; tile < ntiles; tile += nwaves) {
        const long long t0 = tile * BW_TILE - mis;
        const long long tile_lo = t0 > 0 ? t0 : 0, tile_hi = (t0 + BW_TILE < nbytes ? t0 + BW_TILE : nbytes) - 1;
        // first and last record of the tile (the same in every lane)
        const long long r_lo = last_not_above(S.rec_off, first, first + count, base + tile_lo);
        const long long r_hi = S.rec_off[r_lo + 1] > base + tile_hi ? r_lo
                                                                   : last_not_above(S.rec_off, r_lo, first + count, base + tile_hi);
#pragma unroll 1
        for (int k = 0; k < OT_PIECES; ++k) {
            const long long p0 = t0 + (k * 64 + lane) * 16;
            const long long v0 = p0 > 0 ? p0 : 0, v1 = p0 + 16 < nbytes ? p0 + 16 : nbytes;   // head and tail of the range
            if (v0 >= v1) continue;
            const long long r = last_not_above(S.rec_off, r_lo, r_hi + 1, base + v0);
            if (r != R.r) load(r);
            long long q = base + v0 - R.start;
            const bool whole = v1 - v0 == 16;
            const long long sq = BW_FIXED + R.l_name, ql = sq + (R.sl + 1) / 2;
            long long qend = R.len;                             // where QUAL ends
            if constexpr (AUX) {
                qend -= R.al;
                if (whole && q >= qend && q + 16 <= R.len) {    // sixteen bytes of tags
                    *reinterpret_cast<u32x4*>(out + p0) = *reinterpret_cast<const u32x4_unaligned*>(X.aux + R.ao + (q - qend));
                    continue;
                }
            }
            if (whole && q >= ql && q + 16 <= qend) {           // sixteen qualities
                u32x4 v = *reinterpret_cast<const u32x4_unaligned*>(S.qual + R.so + (q - ql));
                v -= 0x21212121u;                               // no borrow between the bytes: the size pass refused values below 33
                *reinterpret_cast<u32x4*>(out + p0) = v;
                continue;
            }
            if (whole && q >= sq && 2 * (q - sq) + 32 <= R.sl) {   // thirty-two bases
                const uint8_t* b = S.seq + R.so + 2 * (q - sq);
                const u32x4 a = *reinterpret_cast<const u32x4_unaligned*>(b);
                const u32x4 c = *reinterpret_cast<const u32x4_unaligned*>(b + 16);
                u32x4 v;
                v.x = pack4(codes4(a.x)) | (pack4(codes4(a.y)) << 16);
                v.y = pack4(codes4(a.z)) | (pack4(codes4(a.w)) << 16);
                v.z = pack4(codes4(c.x)) | (pack4(codes4(c.y)) << 16);
                v.w = pack4(codes4(c.z)) | (pack4(codes4(c.w)) << 16);
                *reinterpret_cast<u32x4*>(out + p0) = v;
                continue;
            }
            // fixed fields, names, the ends of SEQ and QUAL, of records and of the range: byte by byte into the registers
            const int d0 = static_cast<int>(v0 - p0), d1 = static_cast<int>(v1 - p0);
            uint64_t lo = 0, hi = 0;
#pragma unroll 1
            for (int d = d0; d < d1; ++d, ++q) {
                if (q >= R.len) { q = 0; load(R.r + 1); }          // (inside the range: d < d1)
                uint64_t c;
                if constexpr (AUX) c = S.byte_at(R, q, X); else c = S.byte_at(R, q);
                if (d < 8) lo |= c << (8 * d); else hi |= c << (8 * (d - 8));
            }
            if (whole) {
                u32x4 v;
                v.x = static_cast<uint32_t>(lo); v.y = static_cast<uint32_t>(lo >> 32);
                v.z = static_cast<uint32_t>(hi); v.w = static_cast<uint32_t>(hi >> 32);
                *reinterpret_cast<u32x4*>(out + p0) = v;
            } else {
#pragma unroll 1
                for (int d = d0; d < d1; ++d) out[p0 + d] = static_cast<uint8_t>((d < 8 ? lo : hi) >> (8 * (d & 7)));
            }
        }
    }
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

namespace {

template <bool AUX>
int bamw_size(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n, const uint8_t* d_names,
              const int64_t* d_name_off, int64_t first_index, BwAux X, int64_t* d_rec_off, int64_t* d_cuts, int64_t* total_bytes,
              hipStream_t s) {
    return format_size_pass("BAM", "bamw", "bam_format_size", n, d_names, d_name_off, first_index, d_rec_off, total_bytes, s,
        [&](Context& c, long long* d_len, unsigned long long* d_bad) {
            const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(n, OT_THREADS / 64), static_cast<long long>(c.num_cu) * 256));
            hipLaunchKernelGGL(k_bamw_size<AUX>, dim3(grid), dim3(OT_THREADS), 0, s, d_seq, d_qual, d_off, d_names, d_name_off,
                               static_cast<long long>(first_index), static_cast<long long>(n), X, d_len, d_bad);
        },
        [&] {
            if (d_cuts) hipLaunchKernelGGL(k_bamw_cuts<AUX>, dim3(nblk(n, 256)), dim3(256), 0, s, d_off, d_rec_off, X, static_cast<long long>(n), d_cuts);
        },
        [](unsigned long long bad) {
            const long long k = static_cast<long long>(bad >> 20) + 1;
            const unsigned tag = static_cast<unsigned>(bad >> 4) & 0xffffu;
            switch (bad & 15u) {
                case BAMW_NAME_LONG: return fail("record %lld: read name longer than 254 bytes", k);
                case BAMW_NAME_BYTE: return fail("record %lld: read name holds a byte outside '!'..'~'", k);
                case BAMW_BASE: return fail("record %lld: base cannot be stored in BAM", k);
                case BAMW_QUAL: return fail("record %lld: quality byte outside Phred+33", k);
                case BAMW_TAGS: return fail("record %lld: malformed tags", k);
                case BAMW_TAG_TWICE: return fail("record %lld: tag %c%c appears twice", k, static_cast<int>(tag & 255u), static_cast<int>(tag >> 8));
                default: return fail("record %lld: record larger than 2^31 - 1 bytes", k);
            }
        });
}

template <bool AUX>
int bamw_format(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names, const int64_t* d_name_off,
                int64_t first_index, BwAux X, const int64_t* d_rec_off, int64_t first, int64_t count, uint8_t* d_out, hipStream_t s) {
    return format_range("BAM", "bam_format", d_names, d_name_off, first_index, first, count, s, [&](dim3 grid) {
        const BwSource src{d_seq, d_qual, d_off, d_names, d_name_off, static_cast<long long>(first_index), d_rec_off};
        hipLaunchKernelGGL(k_bamw_format<AUX>, grid, dim3(OT_THREADS), 0, s, src, X, static_cast<long long>(first),
                           static_cast<long long>(count), d_out);
    });
}

}  // namespace

extern "C" {

int sarlacc_dev_bam_format_size(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                                const uint8_t* d_names, const int64_t* d_name_off, int64_t first_index,
                                int64_t* d_rec_off, int64_t* d_cuts, int64_t* total_bytes, void* stream) {
    return bamw_size<false>(d_seq, d_qual, d_off, n, d_names, d_name_off, first_index, BwAux{nullptr, nullptr}, d_rec_off, d_cuts,
                            total_bytes, static_cast<hipStream_t>(stream));
}

int sarlacc_dev_bam_format(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names,
                           const int64_t* d_name_off, int64_t first_index, const int64_t* d_rec_off, int64_t first,
                           int64_t count, uint8_t* d_out, void* stream) {
    return bamw_format<false>(d_seq, d_qual, d_off, d_names, d_name_off, first_index, BwAux{nullptr, nullptr}, d_rec_off, first, count,
                              d_out, static_cast<hipStream_t>(stream));
}

int sarlacc_dev_bam_format_size_aux(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                                    const uint8_t* d_names, const int64_t* d_name_off, int64_t first_index,
                                    const uint8_t* d_aux, const int64_t* d_aux_off, int64_t* d_rec_off, int64_t* d_cuts,
                                    int64_t* total_bytes, void* stream) {
    if ((d_aux == nullptr) != (d_aux_off == nullptr)) return fail("sarlacc_amd: tags and their offsets go together");
    if (!d_aux) return sarlacc_dev_bam_format_size(d_seq, d_qual, d_off, n, d_names, d_name_off, first_index, d_rec_off, d_cuts, total_bytes, stream);
    return bamw_size<true>(d_seq, d_qual, d_off, n, d_names, d_name_off, first_index, BwAux{d_aux, d_aux_off}, d_rec_off, d_cuts,
                           total_bytes, static_cast<hipStream_t>(stream));
}

int sarlacc_dev_bam_format_aux(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names,
                               const int64_t* d_name_off, int64_t first_index, const uint8_t* d_aux, const int64_t* d_aux_off,
                               const int64_t* d_rec_off, int64_t first, int64_t count, uint8_t* d_out, void* stream) {
    if ((d_aux == nullptr) != (d_aux_off == nullptr)) return fail("sarlacc_amd: tags and their offsets go together");
    if (!d_aux) return sarlacc_dev_bam_format(d_seq, d_qual, d_off, d_names, d_name_off, first_index, d_rec_off, first, count, d_out, stream);
    return bamw_format<true>(d_seq, d_qual, d_off, d_names, d_name_off, first_index, BwAux{d_aux, d_aux_off}, d_rec_off, first, count,
                             d_out, static_cast<hipStream_t>(stream));
}
}
