// text_lines.hpp -- the line index of newline-separated text in HBM: the tile constants, the unaligned word the byte
// copies use, and the device steps of text_lines.hip.  readers_host.cpp builds the index from them for the FASTQ and
// the SAM reader alike (line_counts, line_starts).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sarlacc {

constexpr int FQ_TILE = 8192;      // bytes per block in the line passes
constexpr int FQ_THREADS = 256;
constexpr int FQ_PER_THREAD = FQ_TILE / FQ_THREADS;  // 32 bytes: two 16-byte loads

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

// device steps (text_lines.hip): one launch each over the ntiles tiles of FQ_TILE bytes that cover the text
int lines_count(const uint8_t* text, long long nbytes, long long ntiles, long long* tile_count, hipStream_t s);
// line_start[k + 1] = position after newline k; tile_base is the exclusive scan of the tile counts
int lines_write(const uint8_t* text, long long nbytes, long long ntiles, const long long* tile_base, long long* line_start,
                hipStream_t s);
// *out = position after newline `target` (1-based); untouched when the text has fewer
int lines_nth_newline(const uint8_t* text, long long nbytes, long long ntiles, const long long* tile_base, long long target,
                      long long* out, hipStream_t s);

}  // namespace sarlacc
