// bam_reads.hip -- BAM alignment records -> resident read batch, on gfx950: SEQ and QUAL of the records (SAM
// specification section 4.2) unpacked into the flat seq / qual / offsets / names layout every other kernel consumes.
// The caller inflates the BGZF blocks on the device (bgzf.hip) and reads the header on the host; the records are
// located by the locator of bam.hip.
//
// A record becomes a read unless flag & exclude_flags.  SEQ holds two 4-bit codes per byte, high nibble first, decoded
// through "=ACMGRSVTWYHKDBN"; QUAL holds Phred values, written as value + 33; with flag & 0x10 the stored read is the
// reverse complement of what was sequenced and is turned back (bases reversed, each code's four bits reversed -- that is
// the complement in this code --, qualities reversed).  A first QUAL byte of 0xff says the record has no qualities.
//
//   k_bamr_size     one wavefront per record: the layout check of k_bam_fields (bam_layout_ok), the keep decision, and
//                   on kept records a scan of SEQ for the code 0 and of QUAL for values above 93, 16 bytes per lane and
//                   step.  It fills keep / bases / name length per record.
//   (rocPRIM exclusive scans over the records: read index, base offset, name offset; k_bamr_reads: read -> record)
//   k_bamr_offsets  d_off / d_name_off of a range of reads, starting at 0
//   k_bamr_unpack   the hot path, divided by OUTPUT bases as k_fqw_format is, not by records (reads run from 200 bases to
//                   100 kb in one batch): a body of out_tiles.hpp's walk_out_tiles over the base offsets of the records
//                   (dropped records have length 0 there), which hands it pieces of 16 bases aligned in memory, so each
//                   store instruction of the wavefront writes 1 KB of consecutive bytes to seq and 1 KB to qual.
//                   A piece inside one read is one unaligned 8-byte load of packed codes (a ninth byte when the piece
//                   starts at an odd base), the nibbles put in base order, the whole 64-bit word bit-reversed for a
//                   reversed read -- which reverses the bases and complements each --, four v_perm_b32 table look-ups
//                   per four letters, and one unaligned 16-byte load of qualities.  A piece that holds the end of a
//                   read or of the range is put together base by base.  Nothing outside the record's SEQ and QUAL is
//                   read, nothing outside the range's bases is written.
//   k_bamr_names    sixteen lanes per record copy its name
//   k_bamr_aux_len / k_bamr_aux_offsets / k_bamr_aux   the tags of the reads (sarlacc_dev_bam_reads_aux_range / _extract):
//                   the bytes behind QUAL of every kept record, sized on the first request for them (a batch read
//                   without tags never pays for it), scanned, and copied as they lie by a walk over OUTPUT bytes
//                   (gather_out_tiles): a move table is kilobytes, a mapper's NM:i:3 four bytes.
//
// No kernel waits on another workgroup, every loop is bounded by a record's own length or the range, and a bad file is an
// error return (first_bad: atomicMin on record << 4 | code), never a fault.
//
// Messages, "BAM record K: <reason>", K 1-based over the alignment records of the file; the lowest record wins, within
// a record layout, SEQ, QUAL; the locator's two messages are those of the ranges path (bam.hip).  The host side -- the
// six sarlacc_dev_bam_reads_* entry points, the index state, these texts -- is in readers_host.cpp; the functions at the
// end of this file only enqueue:
//   layout   record fields do not fit its block size      (every record)
//   seq      SEQ holds '='                                (kept records)
//   qual     quality value above 93                       (kept records)
#include "bam_rec.hpp"
#include "out_tiles.hpp"
#include "readers.hpp"

#include <algorithm>

namespace sarlacc {
namespace {

constexpr int BR_TILE = 64 * 16 * OT_PIECES;      // bases per wavefront and step

// non-zero iff one of the eight nibbles of w is 0
__device__ __forceinline__ uint32_t zero_nibble8(uint32_t w) { return (w - 0x11111111u) & ~w & 0x88888888u; }
// non-zero iff one of the four bytes of w is above 93
__device__ __forceinline__ uint32_t above93_4(uint32_t w) { return (((w & 0x7f7f7f7fu) + 0x22222222u) | w) & 0x80808080u; }

// keep[k], bases[k] = l_seq and name_len[k] of a kept record, 0 of a dropped one
__global__ void __launch_bounds__(OT_THREADS) k_bamr_size(const uint8_t* bam, const long long* rec_off, long long nrec,
                                                          unsigned exclude, int* keep, long long* bases, long long* name_len,
                                                          unsigned long long* first_bad) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = static_cast<long long>(gridDim.x) * (OT_THREADS / 64);
    for (long long k = static_cast<long long>(blockIdx.x) * (OT_THREADS / 64) + (threadIdx.x >> 6); k < nrec; k += nwaves) {
        const uint8_t* rec = bam + rec_off[k];    // block_size >= 32 and wholly in the buffer: the locator checked
        BamFixed F;
        int kept = 0, bad = 0;
        if (!bam_layout_ok(rec, &F)) {
            bad = BAMR_LAYOUT;
        } else if (!(F.flag & exclude)) {
            kept = 1;
            const uint8_t* seq = rec + 36 + F.l_name + 4 * F.n_cig;
            const uint8_t* qual = seq + (F.l_seq + 1) / 2;
            bool eq = wave_any_bad(seq, F.l_seq / 2, lane, [](uint32_t w) { return zero_nibble8(w); },
                                   [](uint8_t c) { return (c & 15) == 0 || (c >> 4) == 0; });
            if ((F.l_seq & 1) && (seq[F.l_seq / 2] >> 4) == 0) eq = true;      // the last byte of an odd read holds one base
            if (eq) bad = BAMR_SEQ;
            else if (F.l_seq > 0 && qual[0] != 0xff && wave_any_bad(qual, F.l_seq, lane, [](uint32_t w) { return above93_4(w); },
                                                                    [](uint8_t c) { return c > 93; })) bad = BAMR_QUAL;
        }
        if (bad) kept = 0;
        if (lane == 0) {
            keep[k] = kept;
            bases[k] = kept ? F.l_seq : 0;
            name_len[k] = kept ? F.l_name - 1 : 0;
            if (bad) atomicMin(first_bad, (static_cast<unsigned long long>(k) << 4) | static_cast<unsigned>(bad));
        }
    }
}

// read_rec[i] = record of read i; read_rec[number of reads] = nrec  (keep[nrec] is 0, read_of[nrec] the number of reads)
__global__ void __launch_bounds__(256) k_bamr_reads(const int* keep, const int64_t* read_of, long long nrec, long long* read_rec) {
    const long long k = blockIdx.x * 256LL + threadIdx.x;
    if (k < nrec ? keep[k] != 0 : k == nrec) read_rec[read_of[k]] = k;
}

// offsets of the reads first .. first + count relative to record a, the record of the first of them
__global__ void __launch_bounds__(256) k_bamr_offsets(const long long* read_rec, const int64_t* base_off, const int64_t* name_off,
                                                      long long first, long long count, long long a, int64_t* d_off,
                                                      int64_t* d_name_off) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i > count) return;
    const long long k = read_rec[first + i];      // (behind the last read of the range: dropped records have no length)
    d_off[i] = base_off[k] - base_off[a];
    if (d_name_off) d_name_off[i] = name_off[k] - name_off[a];
}

// what a lane knows about the read it is writing
struct BrRead {
    long long k = -1, b0 = 0, len = 0;     // record, its first base among all bases of the buffer, its length
    const uint8_t* seq = nullptr;
    const uint8_t* qual = nullptr;
    bool rev = false, missing = false;
};

// letters of the four codes in the low 16 bits of x, first code in the low byte
__device__ __forceinline__ uint32_t letters4(uint32_t x) {
    uint32_t t = (x | (x << 8)) & 0x00ff00ffu;
    t = (t | (t << 4)) & 0x0f0f0f0fu;                        // one code per byte
    const uint32_t sel = t & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(BAM_LETTERS1, BAM_LETTERS0, sel), hi = __builtin_amdgcn_perm(BAM_LETTERS3, BAM_LETTERS2, sel);
    const uint32_t m = ((t >> 3) & 0x01010101u) * 0xffu;     // bytes whose code is 8 or above
    return (hi & m) | (lo & ~m);
}

struct BrSource {
    const uint8_t* bam; const long long* rec_off; const int64_t* base_off;
    uint32_t fill;                         // missing_qual + 33 in every byte

    // a kept record with at least one base (the search for a base returns no other)
    __device__ __forceinline__ void load(BrRead& R, long long k) const {
        R.k = k;
        R.b0 = base_off[k];
        R.len = base_off[k + 1] - R.b0;
        const uint8_t* f = bam + rec_off[k] + 4;
        R.seq = f + 32 + f[8] + 4 * rd_u16(f + 12);
        R.qual = R.seq + (R.len + 1) / 2;
        R.rev = (rd_u16(f + 14) & 16u) != 0;
        R.missing = R.qual[0] == 0xff;
    }

    // base j of the read and its quality
    __device__ __forceinline__ void one(const BrRead& R, long long j, uint8_t* s, uint8_t* q) const {
        const long long i = R.rev ? R.len - 1 - j : j;
        uint32_t c = R.seq[i >> 1];
        c = (i & 1) ? c & 15u : c >> 4;
        if (R.rev) c = __brev(c) >> 28;
        *s = static_cast<uint8_t>((c < 8 ? (static_cast<uint64_t>(BAM_LETTERS1) << 32 | BAM_LETTERS0) : (static_cast<uint64_t>(BAM_LETTERS3) << 32 | BAM_LETTERS2)) >> (8 * (c & 7)));
        *q = R.missing ? static_cast<uint8_t>(fill) : static_cast<uint8_t>(R.qual[i] + 33);
    }

    // bases j .. j + 16 of the read (all inside it) and their qualities
    __device__ __forceinline__ void piece(const BrRead& R, long long j, u32x4* S, u32x4* Q) const {
        const long long s = R.rev ? R.len - 16 - j : j;      // the stored bases s .. s + 16
        const uint8_t* p = R.seq + (s >> 1);
        uint64_t w;
        __builtin_memcpy(&w, p, 8);
        // code of stored base (s & ~1) + i in nibble i: the high nibble of a byte comes first
        uint64_t n = ((w & 0x0f0f0f0f0f0f0f0full) << 4) | ((w >> 4) & 0x0f0f0f0f0f0f0f0full);
        if (s & 1) n = (n >> 4) | (static_cast<uint64_t>(p[8] >> 4) << 60);   // s + 15 is even: the high nibble of the ninth byte
        if (R.rev) n = __brevll(n);        // nibble i <- nibble 15 - i with its bits reversed: reversed and complemented
        S->x = letters4(static_cast<uint32_t>(n) & 0xffffu);
        S->y = letters4(static_cast<uint32_t>(n >> 16) & 0xffffu);
        S->z = letters4(static_cast<uint32_t>(n >> 32) & 0xffffu);
        S->w = letters4(static_cast<uint32_t>(n >> 48));
        if (R.missing) {
            *Q = u32x4{fill, fill, fill, fill};
            return;
        }
        u32x4 v = *reinterpret_cast<const u32x4_unaligned*>(R.qual + s);
        v += 0x21212121u;                  // no carry between the bytes: the size pass refused values above 93
        if (R.rev) v = u32x4{__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x)};
        *Q = v;
    }
};

// seq[0 .. ) and qual[0 .. ) = the bases base_off[a] .. base_off[e] of the buffer: the reads of the records a .. e
__global__ void __launch_bounds__(OT_THREADS) k_bamr_unpack(BrSource S, long long a, long long e, uint8_t* seq, uint8_t* qual) {
    BrRead R;
    walk_out_tiles<OT_THREADS / 64, OT_PIECES>(S.base_off, a, e, seq,
                                               [&](long long base, long long p0, long long v0, long long v1, long long k, long long k_hi) {
        if (k != R.k) S.load(R, k);
        const long long j = base + v0 - R.b0;
        if (v1 - v0 == 16 && j + 16 <= R.len) {
            u32x4 s, q;
            S.piece(R, j, &s, &q);
            *reinterpret_cast<u32x4*>(seq + p0) = s;
            *reinterpret_cast<u32x4_unaligned*>(qual + p0) = q;     // (aligned as well where qual is aligned like seq)
            return;
        }
        // the ends of reads and of the range: base by base
#pragma unroll 1
        for (long long p = v0; p < v1; ++p) {
            if (base + p >= R.b0 + R.len) S.load(R, last_not_above(S.base_off, R.k, k_hi + 1, base + p));
            S.one(R, base + p - R.b0, seq + p, qual + p);
        }
    });
}

// names[0 .. ) = the names of the records a .. e, sixteen lanes per record
__global__ void __launch_bounds__(256) k_bamr_names(const uint8_t* bam, const long long* rec_off, const int64_t* name_off,
                                                    long long a, long long e, uint8_t* names) {
    const int sub = threadIdx.x & 15;
    const long long ngroups = static_cast<long long>(gridDim.x) * 16;
    for (long long k = a + blockIdx.x * 16LL + (threadIdx.x >> 4); k < e; k += ngroups) {
        const long long n = name_off[k + 1] - name_off[k];     // 0 for a dropped record, below 255
        const uint8_t* src = bam + rec_off[k] + 36;
        uint8_t* dst = names + (name_off[k] - name_off[a]);
        for (long long j = sub; j < n; j += 16) dst[j] = src[j];
    }
}

// aux_len[k] = bytes behind QUAL of a kept record, 0 of a dropped one and for k == nrec
__global__ void __launch_bounds__(256) k_bamr_aux_len(const uint8_t* bam, const long long* rec_off, const int* keep, long long nrec,
                                                      long long* aux_len) {
    const long long k = blockIdx.x * 256LL + threadIdx.x;
    if (k > nrec) return;
    long long n = 0;
    if (k < nrec && keep[k]) {
        BamFixed F;
        bam_layout_ok(bam + rec_off[k], &F);      // (it passed in k_bamr_size)
        n = F.bs - (32 + F.l_name + 4 * F.n_cig + (F.l_seq + 1) / 2 + F.l_seq);
    }
    aux_len[k] = n;
}

// aux offsets of the reads first .. first + count relative to record a, the record of the first of them
__global__ void __launch_bounds__(256) k_bamr_aux_offsets(const long long* read_rec, const int64_t* aux_off, long long first,
                                                          long long count, long long a, int64_t* d_aux_off) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i > count) return;
    d_aux_off[i] = aux_off[read_rec[first + i]] - aux_off[a];
}

// aux[0 .. ) = the aux areas of the records a .. e
__global__ void __launch_bounds__(OT_THREADS) k_bamr_aux(const uint8_t* bam, const long long* rec_off, const int64_t* aux_off,
                                                         long long a, long long e, uint8_t* aux) {
    gather_out_tiles(aux_off, a, e, aux, [&](long long k) {
        const uint8_t* rec = bam + rec_off[k];
        return rec + 4 + static_cast<long long>(static_cast<int>(rd_u32(rec))) - (aux_off[k + 1] - aux_off[k]);
    });
}

}  // namespace

int bamr_size(const uint8_t* bam, const long long* rec_off, long long nrec, unsigned exclude, int* keep, long long* bases,
              long long* name_len, unsigned long long* first_bad, hipStream_t s) {
    // one wavefront per record, up to 256 workgroups per CU
    const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(nrec, OT_THREADS / 64), static_cast<long long>(ctx().num_cu) * 256));
    hipLaunchKernelGGL(k_bamr_size, dim3(grid), dim3(OT_THREADS), 0, s, bam, rec_off, nrec, exclude, keep, bases, name_len, first_bad);
    SL_HIP(hipGetLastError());
    return 0;
}

int bamr_reads(const int* keep, const int64_t* read_of, long long nrec, long long* read_rec, hipStream_t s) {
    hipLaunchKernelGGL(k_bamr_reads, dim3(nblk(nrec + 1, 256)), dim3(256), 0, s, keep, read_of, nrec, read_rec);
    SL_HIP(hipGetLastError());
    return 0;
}

int bamr_unpack(const BamrArrays& X, const BamrRange& R, int missing_qual, uint8_t* seq, uint8_t* qual, int64_t* off,
                uint8_t* names, int64_t* name_off, hipStream_t s) {
    const long long num_cu = ctx().num_cu;
    hipLaunchKernelGGL(k_bamr_offsets, dim3(nblk(R.count + 1, 256)), dim3(256), 0, s, X.read_rec, X.base_off, X.name_off, R.first,
                       R.count, R.a, off, name_off);
    SL_HIP(hipGetLastError());
    if (R.bases > 0) {
        const BrSource src{X.bam, X.rec_off, X.base_off, static_cast<uint32_t>(missing_qual + 33) * 0x01010101u};
        const long long ntiles = (R.bases + 15 + BR_TILE - 1) / BR_TILE;
        const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(ntiles, OT_THREADS / 64), num_cu * 8));
        hipLaunchKernelGGL(k_bamr_unpack, dim3(grid), dim3(OT_THREADS), 0, s, src, R.a, R.e, seq, qual);
        SL_HIP(hipGetLastError());
    }
    if (names && R.name_bytes > 0) {
        const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(R.e - R.a, 16), num_cu * 32));
        hipLaunchKernelGGL(k_bamr_names, dim3(grid), dim3(256), 0, s, X.bam, X.rec_off, X.name_off, R.a, R.e, names);
        SL_HIP(hipGetLastError());
    }
    return 0;
}

int bamr_aux_len(const uint8_t* bam, const long long* rec_off, const int* keep, long long nrec, long long* aux_len, hipStream_t s) {
    hipLaunchKernelGGL(k_bamr_aux_len, dim3(nblk(nrec + 1, 256)), dim3(256), 0, s, bam, rec_off, keep, nrec, aux_len);
    SL_HIP(hipGetLastError());
    return 0;
}

int bamr_aux(const BamrArrays& X, const BamrRange& R, uint8_t* aux, int64_t* aux_off, hipStream_t s) {
    hipLaunchKernelGGL(k_bamr_aux_offsets, dim3(nblk(R.count + 1, 256)), dim3(256), 0, s, X.read_rec, X.aux_off, R.first, R.count,
                       R.a, aux_off);
    SL_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bamr_aux, dim3(static_cast<unsigned>(ctx().num_cu) * 8), dim3(OT_THREADS), 0, s, X.bam, X.rec_off, X.aux_off,
                       R.a, R.e, aux);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
