// text_lines.hip -- the line index of newline-separated text in HBM, on gfx950: the kernels that the FASTQ and the SAM
// reader share, each compiled here once.
//
//   k_fq_count        newlines per 8-KB tile                           (reads the text once)
//   (rocPRIM exclusive scan of the tile counts: readers_host.cpp)
//   k_fq_lines        start offset of every line                       (reads the text again)
//   k_fq_nth_newline  end of the k-th record of a block of text (chunked streaming, `number` of adaptorAlign)
//
// The host side -- workspaces, the scan, the sentinels behind the last line -- is line_counts / line_starts of
// readers_host.cpp; the functions at the end of this file only enqueue.
#include "common.hpp"
#include "text_lines.hpp"

namespace sarlacc {

// number of '\n' among the 4 bytes of w
__device__ __forceinline__ int newlines4(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;  // zero byte where '\n'
    int c = 0;
    c += (x & 0x000000ffu) == 0;
    c += (x & 0x0000ff00u) == 0;
    c += (x & 0x00ff0000u) == 0;
    c += (x & 0xff000000u) == 0;
    return c;
}

__device__ __forceinline__ void load32(const uint8_t* text, long long pos, long long nbytes, uint32_t (&w)[8]) {
    if (pos + FQ_PER_THREAD <= nbytes && (reinterpret_cast<uintptr_t>(text + pos) & 15) == 0) {
        const uint4 a = *reinterpret_cast<const uint4*>(text + pos);
        const uint4 b = *reinterpret_cast<const uint4*>(text + pos + 16);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long long p = pos + 4 * k + b;
                if (p < nbytes) v |= static_cast<uint32_t>(text[p]) << (8 * b);
            }
            w[k] = v;
        }
    }
}

__global__ void __launch_bounds__(FQ_THREADS) k_fq_count(const uint8_t* text, long long nbytes, long long* tile_count) {
    const long long pos = static_cast<long long>(blockIdx.x) * FQ_TILE + threadIdx.x * FQ_PER_THREAD;
    int c = 0;
    if (pos < nbytes) {
        uint32_t w[8];
        load32(text, pos, nbytes, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) c += newlines4(w[k]);
    }
    __shared__ int s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = s_sum;
}

// base + the newlines of the tile in front of the thread's 32-byte slot, from the slot's own count c: an exclusive scan
// of the per-thread counts over the block, summed in T (every thread of the block calls it)
template <typename T>
__device__ __forceinline__ T newlines_before(T base, int c) {
    __shared__ int s_wave[FQ_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = base + incl - c;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
    return before;
}

// line_start[k + 1] = position after the k-th newline (0-based); line_start[0] = 0 is set by the host
__global__ void __launch_bounds__(FQ_THREADS) k_fq_lines(const uint8_t* text, long long nbytes, const long long* tile_base,
                                                         long long* line_start) {
    const long long pos = static_cast<long long>(blockIdx.x) * FQ_TILE + threadIdx.x * FQ_PER_THREAD;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int c = 0;
    if (pos < nbytes) {
        load32(text, pos, nbytes, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) c += newlines4(w[k]);
    }
    const int before = newlines_before(0, c);
    if (c == 0) return;
    long long rank = tile_base[blockIdx.x] + before;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (((w[k] >> (8 * b)) & 0xffu) == 0x0au && pos + 4 * k + b < nbytes) {
                line_start[rank + 1] = pos + 4 * k + b + 1;
                ++rank;
            }
        }
    }
}

// position just after newline number `target` (1-based): only the tile that holds it does any work
__global__ void __launch_bounds__(FQ_THREADS) k_fq_nth_newline(const uint8_t* text, long long nbytes, const long long* tile_base,
                                                               long long target, long long* out) {
    const long long before_tile = tile_base[blockIdx.x];
    if (target <= before_tile || target > tile_base[blockIdx.x + 1]) return;   // uniform per block
    const long long pos = static_cast<long long>(blockIdx.x) * FQ_TILE + threadIdx.x * FQ_PER_THREAD;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int c = 0;
    if (pos < nbytes) {
        load32(text, pos, nbytes, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) c += newlines4(w[k]);
    }
    long long rank = newlines_before(before_tile, c);
    if (target <= rank || target > rank + c) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (((w[k] >> (8 * b)) & 0xffu) == 0x0au && pos + 4 * k + b < nbytes) {
                if (++rank == target) *out = pos + 4 * k + b + 1;
            }
        }
    }
}

int lines_count(const uint8_t* text, long long nbytes, long long ntiles, long long* tile_count, hipStream_t s) {
    hipLaunchKernelGGL(k_fq_count, dim3(static_cast<unsigned>(ntiles)), dim3(FQ_THREADS), 0, s, text, nbytes, tile_count);
    SL_HIP(hipGetLastError());
    return 0;
}

int lines_write(const uint8_t* text, long long nbytes, long long ntiles, const long long* tile_base, long long* line_start,
                hipStream_t s) {
    hipLaunchKernelGGL(k_fq_lines, dim3(static_cast<unsigned>(ntiles)), dim3(FQ_THREADS), 0, s, text, nbytes, tile_base, line_start);
    SL_HIP(hipGetLastError());
    return 0;
}

int lines_nth_newline(const uint8_t* text, long long nbytes, long long ntiles, const long long* tile_base, long long target,
                      long long* out, hipStream_t s) {
    hipLaunchKernelGGL(k_fq_nth_newline, dim3(static_cast<unsigned>(ntiles)), dim3(FQ_THREADS), 0, s, text, nbytes, tile_base,
                       target, out);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
