// bam_tags.hip -- the tags of a resident read batch, on gfx950.  A read's tags are the raw aux bytes of its BAM record (SAM
// specification section 4.2.4: everything behind QUAL, in file order, unparsed); a batch holds them flat as names are
// held, d_aux bytes plus n + 1 int64 offsets.  They come from a BAM buffer through sarlacc_dev_bam_reads_aux_range /
// _extract (bam_reads.hip, beside the index state they read) and leave through sarlacc_dev_bam_format_size_aux /
// _format_aux (bam_write.hip).  Here: the query and the one edit kernel.  Every kernel walks entries with bam_rec.hpp's
// bam_tag_next, the whole wavefront on one read.
//
//   k_tags_find     one wavefront per read, strided over a resident grid as k_bamr_size is: the whole aux area of every
//                   read is walked, so the call is also the validator; the first entry whose two tag bytes match is
//                   reported (htslib's bam_aux_get), and how many reads hold it and how many bytes their A / Z / H
//                   values take.
//   k_tags_str_len / (rocPRIM exclusive scan) / k_tags_strings   the A / Z / H values of a find as a flat string set:
//                   a walk over OUTPUT bytes (gather_out_tiles), since MM:Z is kilobytes and RX:Z a dozen bytes.
//   k_tags_ints     the c C s S i I values of a find as int64 and a present mask, one lane per read.
//   k_tags_splice   every edit: output read r is aux[src[r]] without [cut_off[r], cut_off[r] + cut_len[r]), followed by
//                   a new entry built from a column (Z from a flat string set, i from an int32 array) where mask[r].
//                   The host computes the output offsets; the kernel is the same walk over output bytes, a whole piece
//                   inside one of the three sources one unaligned 16-byte load.  What it reads of a source read is
//                   clamped to that read's aux area, whatever the cut arrays say.
//
// No kernel waits on another workgroup; every loop is bounded by a read's aux area or the output range; malformed tags
// are an error return (first_bad: atomicMin), never a fault.
//
// Messages, K 1-based in the batch, the lowest read wins:
//   read K: malformed tags                  (find)
//   read K: tag XX has type T               (strings on a read that holds a number or an array, ints on anything else)
// Out of scope: decoding f and B values (they are kept and written as they lie).
#include "bam_rec.hpp"
#include "out_tiles.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>

namespace sarlacc {
namespace {

__device__ __forceinline__ bool tag_is_string(int t) { return t == 'A' || t == 'Z' || t == 'H'; }
__device__ __forceinline__ bool tag_is_int(int t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }

// per read: the first entry named `tag` (type 0 and zeros when there is none; offsets count from the read's aux start);
// counts[0] += reads that hold it, counts[1] += bytes of their A / Z / H values; first_bad: lowest malformed read
__global__ void __launch_bounds__(OT_THREADS) k_tags_find(const uint8_t* aux, const int64_t* aux_off, long long n, unsigned tag,
                                                          uint8_t* type, int64_t* val_off, int64_t* val_len, int64_t* tag_off,
                                                          int64_t* tag_len, unsigned long long* counts,
                                                          unsigned long long* first_bad) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = static_cast<long long>(gridDim.x) * (OT_THREADS / 64);
    unsigned long long present = 0, sbytes = 0;
    for (long long r = static_cast<long long>(blockIdx.x) * (OT_THREADS / 64) + (threadIdx.x >> 6); r < n; r += nwaves) {
        const long long a0 = aux_off[r], end = aux_off[r + 1] - a0;
        const uint8_t* A = aux + a0;
        BamTag T, hit;
        bool found = false;
        long long p = 0;
        int st;
        while ((st = bam_tag_next(A, p, end, lane, &T)) == BAM_TAG_OK) {      // every turn moves p on by at least 4
            if (!found && T.name == tag) { found = true; hit = T; }
            p = T.next;
        }
        if (st == BAM_TAG_BAD) {
            found = false;
            if (lane == 0) atomicMin(first_bad, static_cast<unsigned long long>(r));
        }
        if (lane == 0 && type) {
            type[r] = found ? static_cast<uint8_t>(hit.type) : 0;
            val_off[r] = found ? hit.val : 0;
            val_len[r] = found ? hit.val_len : 0;
            tag_off[r] = found ? hit.at : 0;
            tag_len[r] = found ? hit.next - hit.at : 0;
        }
        if (found) {
            ++present;
            if (tag_is_string(hit.type)) sbytes += static_cast<unsigned long long>(hit.val_len);
        }
    }
    // one pair of global atomics per workgroup: every wavefront adding to the same two words costs more than the walk
    __shared__ unsigned long long block_counts[2];
    if (threadIdx.x == 0) block_counts[0] = block_counts[1] = 0;
    __syncthreads();
    if (lane == 0 && present) {
        atomicAdd(&block_counts[0], present);
        atomicAdd(&block_counts[1], sbytes);
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_counts[0]) {
        atomicAdd(counts, block_counts[0]);
        atomicAdd(counts + 1, block_counts[1]);
    }
}

// len[r] = bytes of read r's string value, 0 where it has none (len[n] = 0 for the scan); first_bad: read << 8 | type
__global__ void __launch_bounds__(256) k_tags_str_len(const uint8_t* type, const int64_t* val_len, long long n, long long* len,
                                                      unsigned long long* first_bad) {
    const long long r = blockIdx.x * 256LL + threadIdx.x;
    if (r > n) return;
    long long v = 0;
    if (r < n && type[r]) {
        if (tag_is_string(type[r])) v = val_len[r] > 0 ? val_len[r] : 0;
        else atomicMin(first_bad, (static_cast<unsigned long long>(r) << 8) | type[r]);
    }
    len[r] = v;
}

__global__ void __launch_bounds__(OT_THREADS) k_tags_strings(const uint8_t* aux, const int64_t* aux_off, const int64_t* val_off,
                                                             const int64_t* str_off, long long n, uint8_t* chars) {
    gather_out_tiles(str_off, 0, n, chars, [&](long long r) { return aux + aux_off[r] + val_off[r]; });
}

__global__ void __launch_bounds__(256) k_tags_ints(const uint8_t* aux, const int64_t* aux_off, const uint8_t* type,
                                                   const int64_t* val_off, long long n, int64_t* values, uint8_t* present,
                                                   unsigned long long* first_bad) {
    const long long r = blockIdx.x * 256LL + threadIdx.x;
    if (r >= n) return;
    const int t = type[r];
    int64_t v = 0;
    if (tag_is_int(t)) {
        const uint8_t* p = aux + aux_off[r] + val_off[r];
        switch (t) {
            case 'c': v = static_cast<int8_t>(p[0]); break;
            case 'C': v = p[0]; break;
            case 's': v = static_cast<int16_t>(rd_u16(p)); break;
            case 'S': v = rd_u16(p); break;
            case 'i': v = static_cast<int32_t>(rd_u32(p)); break;
            default: v = rd_u32(p); break;
        }
    } else if (t) {
        atomicMin(first_bad, (static_cast<unsigned long long>(r) << 8) | static_cast<unsigned>(t));
    }
    values[r] = v;
    present[r] = tag_is_int(t) ? 1 : 0;
}

struct SpliceSource {
    const uint8_t* aux; const int64_t* aux_off; long long n_src;
    const int64_t* src; const int64_t* cut_off; const int64_t* cut_len;
    unsigned tag; int kind;                      // kind 0: nothing appended, 'Z', 'i'
    const uint8_t* col_chars; const int64_t* col_off; const int32_t* col_ints; const uint8_t* mask;
    const int64_t* out_off;
};

// what a lane knows about the output read it is writing: bytes [0, la) come from pa, [la, la + lb) from pb, the new
// entry of le bytes follows (its Z value: vl bytes at pv), anything behind that (offsets that do not fit) is 0
struct SpliceRead {
    long long r = -1, start = 0, len = 0, la = 0, lb = 0, le = 0, vl = 0;
    const uint8_t* pa = nullptr;
    const uint8_t* pb = nullptr;
    const uint8_t* pv = nullptr;
    uint32_t ival = 0;
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ void splice_load(const SpliceSource& S, SpliceRead& R, long long r) {
    R.r = r;
    R.start = S.out_off[r];
    R.len = S.out_off[r + 1] - R.start;
    const long long s = S.src ? S.src[r] : r;
    long long a0 = 0, alen = 0;
    if (s >= 0 && s < S.n_src) {
        a0 = S.aux_off[s];
        alen = S.aux_off[s + 1] - a0;
        if (alen < 0) alen = 0;
    }
    R.pa = S.aux + a0;
    R.la = alen;
    R.lb = 0;
    R.pb = R.pa;
    if (S.cut_off) {
        const long long co = clampll(S.cut_off[r], 0, alen), cl = clampll(S.cut_len[r], 0, alen - co);
        R.la = co;
        R.pb = R.pa + co + cl;
        R.lb = alen - co - cl;
    }
    R.le = 0; R.vl = 0;
    if (S.kind && (!S.mask || S.mask[r])) {
        if (S.kind == 'Z') {
            const long long vo = S.col_off[r];
            R.vl = S.col_off[r + 1] - vo;
            if (R.vl < 0) R.vl = 0;
            R.pv = S.col_chars + vo;
            R.le = 3 + R.vl + 1;
        } else {
            R.ival = static_cast<uint32_t>(S.col_ints[r]);
            R.le = 7;
        }
    }
}

__device__ __forceinline__ uint8_t splice_byte(const SpliceSource& S, const SpliceRead& R, long long q) {
    if (q < R.la) return R.pa[q];
    q -= R.la;
    if (q < R.lb) return R.pb[q];
    q -= R.lb;
    if (q >= R.le) return 0;
    if (q < 2) return static_cast<uint8_t>(S.tag >> (8 * q));
    if (q == 2) return static_cast<uint8_t>(S.kind);
    q -= 3;
    if (S.kind == 'Z') return q < R.vl ? R.pv[q] : 0;
    return static_cast<uint8_t>(R.ival >> (8 * q));
}

// out[0 .. ) = the output reads 0 .. n_out
__global__ void __launch_bounds__(OT_THREADS) k_tags_splice(SpliceSource S, long long n_out, uint8_t* out) {
    SpliceRead R;
    walk_out_tiles<OT_THREADS / 64, OT_PIECES>(S.out_off, 0, n_out, out,
                                               [&](long long base, long long p0, long long v0, long long v1, long long r, long long) {
        if (r != R.r) splice_load(S, R, r);
        long long q = base + v0 - R.start;
        if (v1 - v0 == 16 && q + 16 <= R.len) {      // a whole piece inside one source
            const uint8_t* from = nullptr;
            const long long qb = q - R.la, qv = qb - R.lb - 3;
            if (q + 16 <= R.la) from = R.pa + q;
            else if (qb >= 0 && qb + 16 <= R.lb) from = R.pb + qb;
            else if (qv >= 0 && qv + 16 <= R.vl) from = R.pv + qv;
            if (from) {
                *reinterpret_cast<u32x4*>(out + p0) = *reinterpret_cast<const u32x4_unaligned*>(from);
                return;
            }
        }
        OutPiece P;
#pragma unroll 1
        for (long long p = v0; p < v1; ++p, ++q) {
            while (q >= R.len) { splice_load(S, R, R.r + 1); q = 0; }      // (inside the range: a read with a byte follows)
            P.put(static_cast<int>(p - p0), splice_byte(S, R, q));
        }
        P.store(out + p0, static_cast<int>(v0 - p0), static_cast<int>(v1 - p0), v1 - v0 == 16);
    });
}

int tag_name_ok(const uint8_t* tag) {
    if (!tag) return fail("sarlacc_amd: a tag name is two bytes");
    return 0;
}

int tag_type_error(unsigned long long bad, const uint8_t* tag) {
    return fail("read %lld: tag %c%c has type %c", static_cast<long long>(bad >> 8) + 1, tag[0], tag[1], static_cast<int>(bad & 255u));
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_bam_tags_find(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n, const uint8_t* tag, uint8_t* d_type,
                              int64_t* d_val_off, int64_t* d_val_len, int64_t* d_tag_off, int64_t* d_tag_len,
                              int64_t* n_present, int64_t* string_bytes, void* stream) {
    SL_TRY(tag_name_ok(tag));
    if (n < 0) return fail("sarlacc_amd: negative number of reads");
    const bool all = d_type && d_val_off && d_val_len && d_tag_off && d_tag_len;
    if (!all && (d_type || d_val_off || d_val_len || d_tag_off || d_tag_len)) return fail("sarlacc_amd: the five results of a tag search go together");
    if (n_present) *n_present = 0;
    if (string_bytes) *string_bytes = 0;
    if (n == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    Context& c = ctx();
    unsigned long long* d_state;      // counts[2], first_bad
    SL_TRY(scratch("bamt.state", 3, &d_state));
    SL_HIP(hipMemsetAsync(d_state, 0, 2 * sizeof(unsigned long long), s));
    SL_HIP(hipMemsetAsync(d_state + 2, 0xff, sizeof(unsigned long long), s));
    c.stage_reset("bam_tags_find");
    SL_TRY(c.stage_begin("bam_tags_find", s));
    const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(n, OT_THREADS / 64), static_cast<long long>(c.num_cu) * 8));
    hipLaunchKernelGGL(k_tags_find, dim3(grid), dim3(OT_THREADS), 0, s, d_aux, d_aux_off, static_cast<long long>(n),
                       tag[0] | (static_cast<unsigned>(tag[1]) << 8), d_type, d_val_off, d_val_len, d_tag_off, d_tag_len, d_state, d_state + 2);
    SL_HIP(hipGetLastError());
    SL_TRY(c.stage_end("bam_tags_find", s));
    unsigned long long state[3];
    SL_HIP(hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (state[2] != ~0ull) return fail("read %lld: malformed tags", static_cast<long long>(state[2]) + 1);
    if (n_present) *n_present = static_cast<int64_t>(state[0]);
    if (string_bytes) *string_bytes = static_cast<int64_t>(state[1]);
    return 0;
}

int sarlacc_dev_bam_tags_strings(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n, const uint8_t* tag,
                                 const uint8_t* d_type, const int64_t* d_val_off, const int64_t* d_val_len, uint8_t* d_chars,
                                 int64_t* d_str_off, void* stream) {
    SL_TRY(tag_name_ok(tag));
    if (n < 0) return fail("sarlacc_amd: negative number of reads");
    hipStream_t s = static_cast<hipStream_t>(stream);
    SL_TRY(ensure_device());
    if (n == 0) {
        SL_HIP(hipMemsetAsync(d_str_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    Context& c = ctx();
    long long* d_len; unsigned long long* d_bad;
    SL_TRY(scratch("bamt.len", static_cast<size_t>(n) + 1, &d_len));
    SL_TRY(scratch("bamt.bad", 1, &d_bad));
    SL_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), s));
    c.stage_reset("bam_tags_strings");
    SL_TRY(c.stage_begin("bam_tags_strings", s));
    hipLaunchKernelGGL(k_tags_str_len, dim3(nblk(n + 1, 256)), dim3(256), 0, s, d_type, d_val_len, static_cast<long long>(n), d_len, d_bad);
    SL_HIP(hipGetLastError());
    SL_TRY(exclusive_scan("bamt.scan", d_len, d_str_off, static_cast<size_t>(n) + 1, s));
    hipLaunchKernelGGL(k_tags_strings, dim3(static_cast<unsigned>(c.num_cu) * 8), dim3(OT_THREADS), 0, s, d_aux, d_aux_off, d_val_off,
                       d_str_off, static_cast<long long>(n), d_chars);
    SL_HIP(hipGetLastError());
    SL_TRY(c.stage_end("bam_tags_strings", s));
    unsigned long long bad = 0;
    SL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) return tag_type_error(bad, tag);
    return 0;
}

int sarlacc_dev_bam_tags_ints(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n, const uint8_t* tag,
                              const uint8_t* d_type, const int64_t* d_val_off, int64_t* d_values, uint8_t* d_present,
                              void* stream) {
    SL_TRY(tag_name_ok(tag));
    if (n < 0) return fail("sarlacc_amd: negative number of reads");
    if (n == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* d_bad;
    SL_TRY(scratch("bamt.bad", 1, &d_bad));
    SL_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_tags_ints, dim3(nblk(n, 256)), dim3(256), 0, s, d_aux, d_aux_off, d_type, d_val_off, static_cast<long long>(n),
                       d_values, d_present, d_bad);
    SL_HIP(hipGetLastError());
    unsigned long long bad = 0;
    SL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) return tag_type_error(bad, tag);
    return 0;
}

int sarlacc_dev_bam_tags_splice(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n_src, const int64_t* d_src, int64_t n_out,
                                const int64_t* d_cut_off, const int64_t* d_cut_len, const uint8_t* tag, int kind,
                                const uint8_t* d_col_chars, const int64_t* d_col_off, const int32_t* d_col_ints,
                                const uint8_t* d_mask, const int64_t* d_out_off, uint8_t* d_out, void* stream) {
    if (n_src < 0 || n_out < 0) return fail("sarlacc_amd: negative number of reads");
    if (n_out == 0) return 0;      // (an empty selection: nothing to write, whatever the other arguments are)
    if (!d_src && n_out != n_src) return fail("sarlacc_amd: a tag splice without 'src' writes every read once");
    if ((d_cut_off == nullptr) != (d_cut_len == nullptr)) return fail("sarlacc_amd: cut offsets and cut lengths go together");
    if (kind != 0 && kind != 'Z' && kind != 'i') return fail("sarlacc_amd: a tag column is of type Z or i");
    if (kind) SL_TRY(tag_name_ok(tag));
    if (kind == 'Z' && (!d_col_chars || !d_col_off)) return fail("sarlacc_amd: a Z column is a flat string set");
    if (kind == 'i' && !d_col_ints) return fail("sarlacc_amd: an i column is an int32 array");
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    Context& c = ctx();
    const SpliceSource src{d_aux, d_aux_off, static_cast<long long>(n_src), d_src, d_cut_off, d_cut_len,
                           kind ? tag[0] | (static_cast<unsigned>(tag[1]) << 8) : 0u, kind, d_col_chars, d_col_off, d_col_ints, d_mask,
                           d_out_off};
    c.stage_reset("bam_tags_splice");
    SL_TRY(c.stage_begin("bam_tags_splice", s));
    hipLaunchKernelGGL(k_tags_splice, dim3(static_cast<unsigned>(c.num_cu) * 8), dim3(OT_THREADS), 0, s, src, static_cast<long long>(n_out), d_out);
    SL_HIP(hipGetLastError());
    SL_TRY(c.stage_end("bam_tags_splice", s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}
}
