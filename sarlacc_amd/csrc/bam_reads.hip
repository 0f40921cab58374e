// bam_reads.hip -- BAM alignment records -> resident read batch, on gfx950: SEQ and QUAL of the records (SAM
// specification section 4.2) unpacked into the flat seq / qual / offsets / names layout every other kernel consumes.
// The caller inflates the BGZF blocks on the device (bgzf.hip) and reads the header on the host; the records are
// located by the locator of bam.hip (bam_locate).
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
// a record layout, SEQ, QUAL; the locator's two messages are bam.hip's:
//   layout   record fields do not fit its block size      (every record)
//   seq      SEQ holds '='                                (kept records)
//   qual     quality value above 93                       (kept records)
#include "bam_rec.hpp"
#include "out_tiles.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>

namespace sarlacc {
namespace {

enum { BAMR_LAYOUT = 1, BAMR_SEQ = 2, BAMR_QUAL = 3 };

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

// state of the last sarlacc_dev_bam_reads_index call on this thread
struct BamReadsIndex {
    bool valid = false;
    const uint8_t* bam = nullptr;
    unsigned long long generation = 0;     // of the locator run whose record offsets this state points to
    long long nrec = 0, nreads = 0, used = 0;
    long long* rec_off = nullptr;          // nrec + 1: the last entry is `used`
    int64_t* base_off = nullptr;           // nrec + 1 each: exclusive scans over the records
    int64_t* name_off = nullptr;
    long long* read_rec = nullptr;         // nreads + 1: record of a read, nrec behind the last
    const int* keep = nullptr;             // nrec + 1
    int64_t* aux_off = nullptr;            // nrec + 1, an exclusive scan as base_off is; null until tags are asked for
};
thread_local BamReadsIndex g_bamr;

// the records a .. e that hold the reads first .. first + count, what they need and where the next record starts
struct BamReadsSpan {
    long long a = 0, e = 0;
    int64_t bases = 0, name_bytes = 0, next_byte = 0;
};

int bamr_span(long long first, long long count, BamReadsSpan* sp);

// the aux offsets of the indexed buffer's records, made on the first request
int bamr_aux_index(hipStream_t s) {
    BamReadsIndex& X = g_bamr;
    if (X.aux_off || X.nrec == 0) return 0;
    long long* d_alen; int64_t* d_aoff;
    SL_TRY(scratch("bamr.alen", static_cast<size_t>(X.nrec) + 1, &d_alen));
    SL_TRY(scratch("bamr.aoff", static_cast<size_t>(X.nrec) + 1, &d_aoff));
    hipLaunchKernelGGL(k_bamr_aux_len, dim3(nblk(X.nrec + 1, 256)), dim3(256), 0, s, X.bam, X.rec_off, X.keep, X.nrec, d_alen);
    SL_HIP(hipGetLastError());
    SL_TRY(exclusive_scan("bamr.scan", d_alen, d_aoff, static_cast<size_t>(X.nrec) + 1, s));
    X.aux_off = d_aoff;
    return 0;
}

int bamr_span(long long first, long long count, BamReadsSpan* sp) {
    const BamReadsIndex& X = g_bamr;
    *sp = BamReadsSpan{};
    if (!X.valid || X.generation != bam_locate_generation())
        return fail("sarlacc_amd: no BAM reads index on this thread (sarlacc_dev_bam_reads_index comes first)");
    if (first < 0 || count < 0 || first > X.nreads || count > X.nreads - first) return fail("sarlacc_amd: BAM read range outside the indexed buffer");
    if (X.nrec == 0) {
        sp->next_byte = X.used;
        return 0;
    }
    // the record after the last read of the range; everything behind the last read of the buffer goes with it
    long long e = 0;
    if (first + count == X.nreads) e = X.nrec;
    else if (first + count > 0) {
        SL_HIP(hipMemcpy(&e, X.read_rec + first + count - 1, sizeof e, hipMemcpyDeviceToHost));
        ++e;
    }
    long long a = e;
    if (count > 0) SL_HIP(hipMemcpy(&a, X.read_rec + first, sizeof a, hipMemcpyDeviceToHost));
    if (a < 0 || a > e || e > X.nrec) return fail("sarlacc_amd: BAM reads index is damaged (internal error)");
    int64_t b[2], n[2];
    long long next = 0;
    SL_HIP(hipMemcpy(&b[0], X.base_off + a, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&b[1], X.base_off + e, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&n[0], X.name_off + a, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&n[1], X.name_off + e, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&next, X.rec_off + e, sizeof next, hipMemcpyDeviceToHost));
    sp->a = a; sp->e = e;
    sp->bases = b[1] - b[0]; sp->name_bytes = n[1] - n[0]; sp->next_byte = next;
    return 0;
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_bam_reads_index(const uint8_t* d_bam, int64_t nbytes, int64_t first_record, int at_eof, int exclude_flags,
                                int64_t* n_records, int64_t* used_bytes, int64_t* n_reads, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0) return fail("sarlacc_amd: negative BAM size");
    if (exclude_flags < 0 || exclude_flags > 0xffff) return fail("'exclude_flags' must lie in 0..65535");
    hipStream_t s = static_cast<hipStream_t>(stream);
    g_bamr = BamReadsIndex{};
    *n_records = 0; *used_bytes = 0; *n_reads = 0;
    if (nbytes == 0) {      // no records: an empty batch
        g_bamr.valid = true; g_bamr.bam = d_bam; g_bamr.generation = bam_locate_generation();
        return 0;
    }
    Context& c = ctx();
    c.stage_reset("bam_reads_size");
    BamLocated L;
    SL_TRY(bam_locate(d_bam, nbytes, s, &L));
    const long long nrec = L.nrec;

    unsigned long long bad = ~0ull;
    int64_t nreads = 0;
    int* d_keep; long long* d_bases; long long* d_nlen; int64_t* d_roff; int64_t* d_boff; int64_t* d_noff; long long* d_rrec;
    unsigned long long* d_bad;
    SL_TRY(scratch("bamr.keep", static_cast<size_t>(nrec) + 1, &d_keep));
    SL_TRY(scratch("bamr.bases", static_cast<size_t>(nrec) + 1, &d_bases));
    SL_TRY(scratch("bamr.nlen", static_cast<size_t>(nrec) + 1, &d_nlen));
    SL_TRY(scratch("bamr.roff", static_cast<size_t>(nrec) + 1, &d_roff));
    SL_TRY(scratch("bamr.boff", static_cast<size_t>(nrec) + 1, &d_boff));
    SL_TRY(scratch("bamr.noff", static_cast<size_t>(nrec) + 1, &d_noff));
    SL_TRY(scratch("bamr.rrec", static_cast<size_t>(nrec) + 1, &d_rrec));
    SL_TRY(scratch("bamr.bad", 1, &d_bad));
    if (nrec > 0) {
        SL_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), s));
        SL_HIP(hipMemsetAsync(d_keep + nrec, 0, sizeof(int), s));
        SL_HIP(hipMemsetAsync(d_bases + nrec, 0, sizeof(long long), s));
        SL_HIP(hipMemsetAsync(d_nlen + nrec, 0, sizeof(long long), s));
        SL_HIP(hipMemcpyAsync(L.d_off + nrec, &L.end, sizeof(long long), hipMemcpyHostToDevice, s));
        const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(nrec, OT_THREADS / 64), static_cast<long long>(c.num_cu) * 256));
        SL_TRY(c.stage_begin("bam_reads_size", s));
        hipLaunchKernelGGL(k_bamr_size, dim3(grid), dim3(OT_THREADS), 0, s, d_bam, L.d_off, nrec, static_cast<unsigned>(exclude_flags),
                           d_keep, d_bases, d_nlen, d_bad);
        SL_HIP(hipGetLastError());
        SL_TRY(exclusive_scan("bamr.scan", d_keep, d_roff, static_cast<size_t>(nrec) + 1, s));
        SL_TRY(exclusive_scan("bamr.scan", d_bases, d_boff, static_cast<size_t>(nrec) + 1, s));
        SL_TRY(exclusive_scan("bamr.scan", d_nlen, d_noff, static_cast<size_t>(nrec) + 1, s));
        hipLaunchKernelGGL(k_bamr_reads, dim3(nblk(nrec + 1, 256)), dim3(256), 0, s, d_keep, d_roff, nrec, d_rrec);
        SL_HIP(hipGetLastError());
        SL_TRY(c.stage_end("bam_reads_size", s));
        SL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
        SL_HIP(hipMemcpyAsync(&nreads, d_roff + nrec, sizeof nreads, hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
    }
    if (bad != ~0ull) {      // a record before the one the chain ends at: the lowest record wins
        const long long k = first_record + static_cast<long long>(bad >> 4);
        switch (bad & 15u) {
            case BAMR_LAYOUT: return fail("BAM record %lld: record fields do not fit its block size", k);
            case BAMR_SEQ: return fail("BAM record %lld: SEQ holds '='", k);
            default: return fail("BAM record %lld: quality value above 93", k);
        }
    }
    SL_TRY(bam_chain_end_error(L, first_record, at_eof));
    BamReadsIndex& X = g_bamr;
    X.valid = true; X.bam = d_bam; X.generation = L.generation;
    X.nrec = nrec; X.nreads = nreads; X.used = L.end;
    X.rec_off = L.d_off; X.base_off = d_boff; X.name_off = d_noff; X.read_rec = d_rrec; X.keep = d_keep;
    *n_records = nrec; *used_bytes = L.end; *n_reads = nreads;
    return 0;
}

int sarlacc_dev_bam_reads_range(int64_t first, int64_t count, int64_t* total_bases, int64_t* total_name_bytes,
                                int64_t* next_byte) {
    BamReadsSpan sp;
    SL_TRY(bamr_span(first, count, &sp));
    *total_bases = sp.bases; *total_name_bytes = sp.name_bytes; *next_byte = sp.next_byte;
    return 0;
}

int sarlacc_dev_bam_reads_records(int64_t reads_taken, int64_t* n_records) {
    BamReadsSpan sp;
    SL_TRY(bamr_span(0, reads_taken, &sp));
    *n_records = sp.e;
    return 0;
}

int sarlacc_dev_bam_reads_extract(const uint8_t* d_bam, int64_t first, int64_t count, int missing_qual, uint8_t* d_seq,
                                  uint8_t* d_qual, int64_t* d_off, uint8_t* d_names, int64_t* d_name_off, void* stream) {
    if (missing_qual < 0 || missing_qual > 93) return fail("'missing_qual' must lie in 0..93");
    if ((d_names == nullptr) != (d_name_off == nullptr)) return fail("sarlacc_amd: read names and their offsets go together");
    BamReadsSpan sp;
    SL_TRY(bamr_span(first, count, &sp));
    const BamReadsIndex& X = g_bamr;
    if (d_bam != X.bam) return fail("sarlacc_amd: not the BAM buffer indexed last on this thread");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count == 0 || X.nrec == 0) {      // offsets that start at 0, and nothing else
        SL_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), s));
        if (d_name_off) SL_HIP(hipMemsetAsync(d_name_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    Context& c = ctx();
    c.stage_reset("bam_reads_unpack");
    SL_TRY(c.stage_begin("bam_reads_unpack", s));
    hipLaunchKernelGGL(k_bamr_offsets, dim3(nblk(count + 1, 256)), dim3(256), 0, s, X.read_rec, X.base_off, X.name_off,
                       static_cast<long long>(first), static_cast<long long>(count), sp.a, d_off, d_name_off);
    SL_HIP(hipGetLastError());
    if (sp.bases > 0) {
        const BrSource src{d_bam, X.rec_off, X.base_off, static_cast<uint32_t>(missing_qual + 33) * 0x01010101u};
        const long long ntiles = (sp.bases + 15 + BR_TILE - 1) / BR_TILE;
        const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(ntiles, OT_THREADS / 64), static_cast<long long>(c.num_cu) * 8));
        hipLaunchKernelGGL(k_bamr_unpack, dim3(grid), dim3(OT_THREADS), 0, s, src, sp.a, sp.e, d_seq, d_qual);
        SL_HIP(hipGetLastError());
    }
    if (d_names && sp.name_bytes > 0) {
        const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(sp.e - sp.a, 16), static_cast<long long>(c.num_cu) * 32));
        hipLaunchKernelGGL(k_bamr_names, dim3(grid), dim3(256), 0, s, d_bam, X.rec_off, X.name_off, sp.a, sp.e, d_names);
        SL_HIP(hipGetLastError());
    }
    SL_TRY(c.stage_end("bam_reads_unpack", s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

int sarlacc_dev_bam_reads_aux_range(int64_t first, int64_t count, int64_t* aux_bytes) {
    BamReadsSpan sp;
    SL_TRY(bamr_span(first, count, &sp));
    *aux_bytes = 0;
    if (count == 0 || g_bamr.nrec == 0) return 0;
    SL_TRY(bamr_aux_index(nullptr));
    int64_t b[2];
    SL_HIP(hipMemcpy(&b[0], g_bamr.aux_off + sp.a, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&b[1], g_bamr.aux_off + sp.e, sizeof(int64_t), hipMemcpyDeviceToHost));
    *aux_bytes = b[1] - b[0];
    return 0;
}

int sarlacc_dev_bam_reads_aux_extract(const uint8_t* d_bam, int64_t first, int64_t count, uint8_t* d_aux, int64_t* d_aux_off,
                                      void* stream) {
    BamReadsSpan sp;
    SL_TRY(bamr_span(first, count, &sp));
    BamReadsIndex& X = g_bamr;
    if (d_bam != X.bam) return fail("sarlacc_amd: not the BAM buffer indexed last on this thread");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count == 0 || X.nrec == 0) {
        SL_HIP(hipMemsetAsync(d_aux_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    SL_TRY(bamr_aux_index(s));
    Context& c = ctx();
    c.stage_reset("bam_reads_aux");
    SL_TRY(c.stage_begin("bam_reads_aux", s));
    hipLaunchKernelGGL(k_bamr_aux_offsets, dim3(nblk(count + 1, 256)), dim3(256), 0, s, X.read_rec, X.aux_off,
                       static_cast<long long>(first), static_cast<long long>(count), sp.a, d_aux_off);
    SL_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bamr_aux, dim3(static_cast<unsigned>(c.num_cu) * 8), dim3(OT_THREADS), 0, s, d_bam, X.rec_off, X.aux_off,
                       sp.a, sp.e, d_aux);
    SL_HIP(hipGetLastError());
    SL_TRY(c.stage_end("bam_reads_aux", s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}
}
