// text_lines.hpp -- the line index of newline-separated text in HBM, shared by the FASTQ (fastq.hip) and SAM
// (sam.hip) parsers:
//
//   k_fq_count    newlines per 8-KB tile                           (reads the text once)
//   (rocPRIM exclusive scan of the tile counts)
//   k_fq_lines    start offset of every line                       (reads the text again)
//
// Everything here has internal linkage (anonymous namespace): each translation unit that includes the header gets its
// own copy of the kernels, so the objects do not clash at link time.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sarlacc {
namespace {

constexpr int FQ_TILE = 8192;      // bytes per block in the line passes
constexpr int FQ_THREADS = 256;
constexpr int FQ_PER_THREAD = FQ_TILE / FQ_THREADS;  // 32 bytes: two 16-byte loads

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

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
    // exclusive scan of the per-thread counts over the block
    __shared__ int s_wave[FQ_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = incl - c;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
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

}  // namespace
}  // namespace sarlacc
