// out_tiles.hpp -- what the kernels that write a record range by OUTPUT bytes share (fastq_write.hip k_fqw_format,
// bam_reads.hip k_bamr_unpack; bam_write.hip k_bamw_format keeps a copy of the walk and the piece in its body, for its
// registers' sake, and changes with them), their size passes, and the host side of the two writers.
//
// Records run from nothing to tens of kilobases in one batch, so the work is divided by the bytes written, not by
// records.  A wavefront takes tiles of 4 KB of the output, every lane four 16-byte pieces of a tile, 1 KB apart, so that
// each store instruction of the wavefront writes 1 KB of consecutive addresses.  Pieces are aligned in MEMORY, not in
// the output: the destination's misalignment shifts the tiles, and the first and the last piece of a range may be cut
// (the head and the tail).  A tile finds its first and last record by binary search in the n + 1 record offsets, a lane
// searches only between those two.  walk_out_tiles is that walk; a kernel says what a piece is.
//
// Everything here has internal linkage (anonymous namespace): every file that includes it gets its own copy.
#pragma once

#include "common.hpp"
#include "devprim.hpp"

#include <string>

namespace sarlacc {
namespace {

constexpr int OT_THREADS = 256;                   // the walk kernels' workgroup
constexpr int OT_PIECES = 4;                      // 16-byte pieces per lane and tile
constexpr int NAME_PREFIX = 5;                    // "READ_"

typedef uint32_t __attribute__((ext_vector_type(4))) u32x4;
typedef u32x4 __attribute__((aligned(1))) u32x4_unaligned;

// piece(base, p0, v0, v1, r, r_hi) for every non-empty piece of the output bytes off[first] .. off[last] that the
// wavefront owns, in a grid of workgroups of WAVES wavefronts: base = off[first]; the piece is the 16 bytes from p0 of
// the range, of which [v0, v1) lie inside it (p0 < 0 in the head, v1 - v0 < 16 there and in the tail); dst + p0 is
// 16-byte aligned; r is the record that holds byte v0, r_hi the last record of the tile.
template <int WAVES, int PIECES, typename Piece>
__device__ __forceinline__ void walk_out_tiles(const int64_t* off, long long first, long long last, const void* dst, Piece&& piece) {
    constexpr int TILE = 64 * 16 * PIECES;
    const long long base = off[first], nbytes = off[last] - base;
    const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 15);
    const long long ntiles = (nbytes + mis + TILE - 1) / TILE;
    const int lane = threadIdx.x & 63;
    const long long wave = blockIdx.x * static_cast<long long>(WAVES) + (threadIdx.x >> 6);
    const long long nwaves = static_cast<long long>(gridDim.x) * WAVES;
    for (long long tile = wave; tile < ntiles; tile += nwaves) {
        const long long t0 = tile * TILE - mis;
        const long long tile_lo = t0 > 0 ? t0 : 0, tile_hi = (t0 + TILE < nbytes ? t0 + TILE : nbytes) - 1;
        // first and last record of the tile (the same in every lane)
        const long long r_lo = last_not_above(off, first, last, base + tile_lo);
        const long long r_hi = off[r_lo + 1] > base + tile_hi ? r_lo : last_not_above(off, r_lo, last, base + tile_hi);
#pragma unroll 1
        for (int k = 0; k < PIECES; ++k) {
            const long long p0 = t0 + (k * 64 + lane) * 16;
            const long long v0 = p0 > 0 ? p0 : 0, v1 = p0 + 16 < nbytes ? p0 + 16 : nbytes;   // head and tail of the range
            if (v0 >= v1) continue;
            piece(base, p0, v0, v1, last_not_above(off, r_lo, r_hi + 1, base + v0), r_hi);
        }
    }
}

// the 16 bytes a lane puts together before it stores them
struct OutPiece {
    uint64_t lo = 0, hi = 0;

    __device__ __forceinline__ void put(int d, uint8_t c) {
        if (d < 8) lo |= static_cast<uint64_t>(c) << (8 * d); else hi |= static_cast<uint64_t>(c) << (8 * (d - 8));
    }

    // bytes [d0, d1) to p (16-byte aligned): one store of a whole piece, byte by byte at the two ends of a range
    __device__ __forceinline__ void store(uint8_t* p, int d0, int d1, bool whole) const {
        if (whole) {
            u32x4 v;
            v.x = static_cast<uint32_t>(lo); v.y = static_cast<uint32_t>(lo >> 32);
            v.z = static_cast<uint32_t>(hi); v.w = static_cast<uint32_t>(hi >> 32);
            *reinterpret_cast<u32x4*>(p) = v;
        } else {
#pragma unroll 1
            for (int d = d0; d < d1; ++d) p[d] = static_cast<uint8_t>((d < 8 ? lo : hi) >> (8 * (d & 7)));
        }
    }
};

// out[0 .. ) = the bytes off[first] .. off[last] of a flat layout whose record r lies at src(r)[0 .. off[r + 1] - off[r]):
// a whole piece inside one record is one unaligned 16-byte load, anything else is put together byte by byte.  src is
// asked for empty records too and must not read through the pointer it returns.
template <typename Src>
__device__ __forceinline__ void gather_out_tiles(const int64_t* off, long long first, long long last, uint8_t* out, Src&& src) {
    long long cur = -1, start = 0, len = 0;
    const uint8_t* sp = nullptr;
    walk_out_tiles<OT_THREADS / 64, OT_PIECES>(off, first, last, out,
                                               [&](long long base, long long p0, long long v0, long long v1, long long r, long long) {
        if (r != cur) { cur = r; start = off[r]; len = off[r + 1] - start; sp = src(r); }
        long long q = base + v0 - start;
        if (v1 - v0 == 16 && q + 16 <= len) {
            *reinterpret_cast<u32x4*>(out + p0) = *reinterpret_cast<const u32x4_unaligned*>(sp + q);
            return;
        }
        OutPiece P;
#pragma unroll 1
        for (long long p = v0; p < v1; ++p, ++q) {
            while (q >= len) {         // (inside the range: a record with a byte follows)
                ++cur; start = off[cur]; len = off[cur + 1] - start; sp = src(cur); q = 0;
            }
            P.put(static_cast<int>(p - p0), sp[q]);
        }
        P.store(out + p0, static_cast<int>(v0 - p0), static_cast<int>(v1 - p0), v1 - v0 == 16);
    });
}

__device__ __forceinline__ int decimal_width(unsigned long long v) {
    int w = 1;
    while (v >= 10) { v /= 10; ++w; }
    return w;
}

// character k of the default name READ_<v>, a name of len bytes
template <typename I>
__device__ __forceinline__ uint8_t default_name_char(unsigned long long v, I len, I k) {
    if (k < NAME_PREFIX) return static_cast<uint8_t>("READ_"[k]);
    for (I d = len - 1 - k; d > 0; --d) v /= 10;   // digit k - 5 of len - 5, from the left
    return static_cast<uint8_t>('0' + v % 10);
}

// whether one of the n bytes at p is bad: the whole wavefront, 16 bytes per lane and step through bad4 (non-zero iff one
// of a word's four bytes is bad), the last bytes one by one through bad1
template <typename Bad4, typename Bad1>
__device__ __forceinline__ bool wave_any_bad(const uint8_t* p, long long n, int lane, Bad4 bad4, Bad1 bad1) {
    bool hit = false;
    for (long long q = 16LL * lane; q < n; q += 16 * 64) {
        if (q + 16 <= n) {
            const u32x4 v = *reinterpret_cast<const u32x4_unaligned*>(p + q);
            hit |= (bad4(v.x) | bad4(v.y) | bad4(v.z) | bad4(v.w)) != 0;
        } else {
            for (long long j = q; j < n; ++j) hit |= bad1(p[j]);
        }
    }
    return __ballot(hit) != 0;
}

// Host side of a writer `what` ("FASTQ", "BAM") whose scratch buffers are <tag>.len, <tag>.bad and <tag>.scan.
inline int format_request_ok(const char* what, bool numbers_ok, const uint8_t* d_names, const int64_t* d_name_off) {
    if (!numbers_ok) return fail("sarlacc_amd: bad %s format request", what);
    if ((d_names == nullptr) != (d_name_off == nullptr)) return fail("sarlacc_amd: read names and their offsets go together");
    return 0;
}

// The size pass under the stage timer `stage`: launch(ctx, len, first_bad) fills the n + 1 record lengths (the last one 0)
// and lowers *first_bad from ~0 for a record it refuses; their exclusive scan is d_rec_off; after_scan() launches what
// reads it; the total comes to the host, or message(first_bad) is the error.
template <typename Launch, typename AfterScan, typename Message>
int format_size_pass(const char* what, const std::string& tag, const char* stage, int64_t n, const uint8_t* d_names,
                     const int64_t* d_name_off, int64_t first_index, int64_t* d_rec_off, int64_t* total_bytes, hipStream_t s,
                     Launch launch, AfterScan after_scan, Message message) {
    SL_TRY(format_request_ok(what, n >= 0 && first_index >= 0 && total_bytes, d_names, d_name_off));
    SL_TRY(ensure_device());
    *total_bytes = 0;
    if (n == 0) {
        SL_HIP(hipMemsetAsync(d_rec_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    Context& c = ctx();
    long long* d_len; unsigned long long* d_bad;
    SL_TRY(scratch(tag + ".len", static_cast<size_t>(n) + 1, &d_len));
    SL_TRY(scratch(tag + ".bad", 1, &d_bad));
    SL_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), s));
    c.stage_reset(stage);
    SL_TRY(c.stage_begin(stage, s));
    launch(c, d_len, d_bad);
    SL_HIP(hipGetLastError());
    SL_TRY(exclusive_scan(tag + ".scan", d_len, d_rec_off, static_cast<size_t>(n) + 1, s));
    after_scan();
    SL_HIP(hipGetLastError());
    SL_TRY(c.stage_end(stage, s));
    unsigned long long bad = 0;
    int64_t total = 0;
    SL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipMemcpyAsync(&total, d_rec_off + n, sizeof total, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) return message(bad);
    *total_bytes = total;
    return 0;
}

// The format pass of a record range under the stage timer `stage`: launch(grid) starts the walk kernel.  The size of the
// range is known on the device only: a resident grid whose wavefronts stride over the tiles.
template <typename Launch>
int format_range(const char* what, const char* stage, const uint8_t* d_names, const int64_t* d_name_off, int64_t first_index,
                 int64_t first, int64_t count, hipStream_t s, Launch launch) {
    SL_TRY(format_request_ok(what, first >= 0 && count >= 0 && first_index >= 0, d_names, d_name_off));
    if (count == 0) return 0;
    SL_TRY(ensure_device());
    Context& c = ctx();
    c.stage_reset(stage);
    SL_TRY(c.stage_begin(stage, s));
    launch(dim3(static_cast<unsigned>(c.num_cu) * 8));
    SL_HIP(hipGetLastError());
    SL_TRY(c.stage_end(stage, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace
}  // namespace sarlacc
