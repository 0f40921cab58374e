// fastq_write.hip -- resident read batch -> FASTQ text, on gfx950: the inverse of fastq.hip's sarlacc_dev_fastq_extract.
//
// The reference leaves the library through FASTQ files (writeXStringSet on realizeReads' output and on the consensus
// reads, vignettes/correction.Rmd:271-278, :352).  Here the text is formatted in HBM from the flat
// layout the other kernels use and comes back to the host as one contiguous block.  Record i is
//
//     '@' name '\n' seq '\n' '+' '\n' qual '\n'          (LF only; name_len + 2 L + 6 bytes)
//
// with the default name READ_<first_index + i> (decimal, unpadded) when the batch has no names.
//
//   k_fqw_size    byte length of every record; refuses names that hold '\n' or '\r'   (reads offsets and names)
//   (rocPRIM exclusive scan: n + 1 record offsets, the last one is the size of the text)
//   k_fqw_format  the text of a contiguous record range                               (reads seq, qual, names once; writes the text once)
//
// k_fqw_format divides the work by OUTPUT bytes, not by records: it is a body of out_tiles.hpp's walk_out_tiles, which
// hands it 16-byte pieces of the text, aligned in memory, with the record each starts in.
// A piece that lies inside one name, sequence or quality string is one unaligned 16-byte load --
// source and destination are misaligned against each other by a different amount for every record and string, so the
// loads are the unaligned side --; a piece that holds a separator, the digits of a default name, a string's first or last
// bytes or the ends of the text is put together byte by byte.
//
// Compressed output is bgzf_deflate.hip's, on the text this file leaves in device memory.
// Out of scope: multi-line FASTQ, a repeated name on the '+' line.
#include "out_tiles.hpp"

#include "../../include/sarlacc_amd.h"

namespace sarlacc {
namespace {

// non-zero iff one of the four bytes of w is '\n' or '\r'
__device__ __forceinline__ uint32_t line_break4(uint32_t w) {
    const uint32_t a = w ^ 0x0a0a0a0au, b = w ^ 0x0d0d0d0du;
    return (((a - 0x01010101u) & ~a) | ((b - 0x01010101u) & ~b)) & 0x80808080u;
}

// len[r] = bytes of record r (len[n] = 0 for the scan); first_bad: lowest record whose name holds a line break
__global__ void __launch_bounds__(256) k_fqw_size(const int64_t* off, const uint8_t* names, const int64_t* name_off,
                                                  long long first_index, long long n, long long* len,
                                                  unsigned long long* first_bad) {
    const long long tid = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    const long long nthreads = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long r = tid; r < n; r += nthreads) {
        const long long nl = names ? name_off[r + 1] - name_off[r]
                                   : NAME_PREFIX + decimal_width(static_cast<unsigned long long>(first_index + r));
        len[r] = nl + 2 * (off[r + 1] - off[r]) + 6;
    }
    if (tid == 0) len[n] = 0;
    if (!names) return;
    // the name bytes, 16 per thread and step
    const long long nb0 = name_off[0], nb1 = name_off[n];
    for (long long p = nb0 + 16 * tid; p < nb1; p += 16 * nthreads) {
        const int k = static_cast<int>(nb1 - p < 16 ? nb1 - p : 16);
        if (k == 16) {
            const u32x4 v = *reinterpret_cast<const u32x4_unaligned*>(names + p);
            if (!(line_break4(v.x) | line_break4(v.y) | line_break4(v.z) | line_break4(v.w))) continue;
        }
        for (int j = 0; j < k; ++j) {
            const uint8_t c = names[p + j];
            if (c == '\n' || c == '\r') {   // the first one of the piece: positions grow with the records
                atomicMin(first_bad, static_cast<unsigned long long>(last_not_above(name_off, 0, n, p + j)));
                break;
            }
        }
    }
}

// what a lane knows about the record it is writing
struct FwRec {
    long long r = -1, start = 0, len = 0;    // record, its first byte in the whole text, its length
    long long so = 0, sl = 0, no = 0, nl = 0;   // sequence / quality offset and length, name offset and length
};

// bits of the bytes [a, b) of a 64-bit word (a, b clamped to 0 .. 8)
__device__ __forceinline__ uint64_t byte_mask(int a, int b) {
    a = a < 0 ? 0 : a;
    b = b > 8 ? 8 : b;
    if (a >= b) return 0;
    return (b - a == 8 ? ~0ull : (1ull << (8 * (b - a))) - 1) << (8 * a);
}

// OutPiece, and whole strings into it
struct FwPiece : OutPiece {
    // bytes [d, d + m) = bytes [x, x + m) of the string s of len bytes.  One unaligned 16-byte load that stays inside the
    // string, shifted to its place; a string shorter than that byte by byte.
    __device__ __forceinline__ void put_string(int d, int m, const uint8_t* s, long long len, long long x) {
        if (len < 16) {
            for (int k = 0; k < m; ++k) put(d + k, s[x + k]);
            return;
        }
        long long y = x - d;
        y = y < 0 ? 0 : y;
        y = y > len - 16 ? len - 16 : y;
        const u32x4 v = *reinterpret_cast<const u32x4_unaligned*>(s + y);
        uint64_t a = v.x | static_cast<uint64_t>(v.y) << 32, b = v.z | static_cast<uint64_t>(v.w) << 32;
        const int up = d - static_cast<int>(x - y);   // bytes towards the end of the piece, -15 .. 15
        if (up >= 8) { b = a << (8 * (up - 8)); a = 0; }
        else if (up > 0) { b = (b << (8 * up)) | (a >> (64 - 8 * up)); a <<= 8 * up; }
        else if (up <= -8) { a = b >> (8 * (-up - 8)); b = 0; }
        else if (up < 0) { a = (a >> (8 * -up)) | (b << (64 + 8 * up)); b >>= 8 * -up; }
        lo |= a & byte_mask(d, d + m);
        hi |= b & byte_mask(d - 8, d + m - 8);
    }
};

struct FwSource {
    const uint8_t* seq; const uint8_t* qual; const int64_t* off;
    const uint8_t* names; const int64_t* name_off; long long first_index;
    const int64_t* rec_off;

    __device__ __forceinline__ void load(FwRec& R, long long r) const {
        R.r = r;
        R.start = rec_off[r];
        R.len = rec_off[r + 1] - R.start;
        R.so = off[r];
        R.sl = off[r + 1] - R.so;
        if (names) { R.no = name_off[r]; R.nl = name_off[r + 1] - R.no; }
        else R.nl = R.len - 2 * R.sl - 6;
    }

    // the string 16 consecutive bytes of record R from byte q lie in, or null
    __device__ __forceinline__ const uint8_t* inside(const FwRec& R, long long q) const {
        long long b = 1;                             // the name
        if (names && q >= b && q + 16 <= b + R.nl) return names + R.no + (q - b);
        b += R.nl + 1;                               // the sequence
        if (q >= b && q + 16 <= b + R.sl) return seq + R.so + (q - b);
        b += R.sl + 3;                               // the qualities
        if (q >= b && q + 16 <= b + R.sl) return qual + R.so + (q - b);
        return nullptr;
    }

    // bytes [d, d + m) of the piece = bytes [q, q + m) of record R (all of them inside the record)
    __device__ __forceinline__ void part(FwPiece& P, int d, int m, const FwRec& R, long long q) const {
        const long long name = 1, after_name = name + R.nl, sq = after_name + 1, after_seq = sq + R.sl, ql = after_seq + 3;
        const long long sep[6] = {0, after_name, after_seq, after_seq + 1, after_seq + 2, R.len - 1};
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (sep[k] >= q && sep[k] < q + m) P.put(d + static_cast<int>(sep[k] - q), k == 0 ? '@' : k == 3 ? '+' : '\n');
        const long long begin[3] = {name, sq, ql}, len[3] = {R.nl, R.sl, R.sl};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long a = q > begin[k] ? q : begin[k], e = q + m < begin[k] + len[k] ? q + m : begin[k] + len[k];
            if (a >= e) continue;
            const int dd = d + static_cast<int>(a - q), mm = static_cast<int>(e - a);
            if (k == 0 && !names) {
                for (int c = 0; c < mm; ++c) P.put(dd + c, default_name_char(static_cast<unsigned long long>(first_index + R.r), R.nl, a - name + c));
            } else {
                P.put_string(dd, mm, k == 0 ? names + R.no : (k == 1 ? seq : qual) + R.so, len[k], a - begin[k]);
            }
        }
    }
};

// text[0 .. ) = bytes rec_off[first] .. rec_off[first + count] of the whole text
__global__ void __launch_bounds__(OT_THREADS) k_fqw_format(FwSource S, long long first, long long count, uint8_t* text) {
    FwRec R;
    walk_out_tiles<OT_THREADS / 64, OT_PIECES>(S.rec_off, first, first + count, text,
                                               [&](long long base, long long p0, long long v0, long long v1, long long r, long long) {
        if (r != R.r) S.load(R, r);
        long long q = base + v0 - R.start;
        const bool whole = v1 - v0 == 16;
        const uint8_t* src = whole ? S.inside(R, q) : nullptr;
        if (src) {
            *reinterpret_cast<u32x4*>(text + p0) = *reinterpret_cast<const u32x4_unaligned*>(src);
            return;
        }
        // separators, default names, the ends of strings, of records and of the text: record by record
        const int d0 = static_cast<int>(v0 - p0), d1 = static_cast<int>(v1 - p0);
        FwPiece P;
#pragma unroll 1
        for (int d = d0; d < d1;) {
            if (q >= R.len) { q = 0; S.load(R, R.r + 1); }
            const int m = static_cast<int>(R.len - q < d1 - d ? R.len - q : d1 - d);
            S.part(P, d, m, R, q);
            d += m;
            q += m;
        }
        P.store(text + p0, d0, d1, whole);
    });
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_fastq_format_size(const int64_t* d_off, int64_t n, const uint8_t* d_names, const int64_t* d_name_off,
                                  int64_t first_index, int64_t* d_rec_off, int64_t* total_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    return format_size_pass("FASTQ", "fqw", "fastq_size", n, d_names, d_name_off, first_index, d_rec_off, total_bytes, s,
        [&](Context&, long long* d_len, unsigned long long* d_bad) {
            hipLaunchKernelGGL(k_fqw_size, dim3(nblk(n, 256)), dim3(256), 0, s, d_off, d_names, d_name_off,
                               static_cast<long long>(first_index), static_cast<long long>(n), d_len, d_bad);
        },
        [] {},
        [](unsigned long long bad) { return fail("record %lld: read name holds a line break", static_cast<long long>(bad) + 1); });
}

int sarlacc_dev_fastq_format(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names,
                             const int64_t* d_name_off, int64_t first_index, const int64_t* d_rec_off, int64_t first,
                             int64_t count, uint8_t* d_text, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    return format_range("FASTQ", "fastq_format", d_names, d_name_off, first_index, first, count, s, [&](dim3 grid) {
        const FwSource src{d_seq, d_qual, d_off, d_names, d_name_off, static_cast<long long>(first_index), d_rec_off};
        hipLaunchKernelGGL(k_fqw_format, grid, dim3(OT_THREADS), 0, s, src, static_cast<long long>(first),
                           static_cast<long long>(count), d_text);
    });
}
}
