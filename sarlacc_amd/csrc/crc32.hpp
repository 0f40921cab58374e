// crc32.hpp -- CRC-32 arithmetic (the polynomial of RFC 1952, reflected) shared by the BGZF reader (bgzf.hip) and
// writer (bgzf_deflate.hip): a table entry, and the shift that lets slices of a block be summed independently and
// folded (crc(A B) = crc(A) x^(8 |B|) + crc(B)).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sarlacc {

constexpr uint32_t CRC_POLY = 0xedb88320u;

// a(x) * b(x) mod p(x), bit 31 = x^0 (zlib's multmodp)
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// the CRC of A followed by `nbytes` more bytes, as far as A's CRC goes: crc(A) * x^(8 nbytes)
__host__ __device__ inline uint32_t crc_shift(uint32_t crc, uint32_t nbytes) {
    uint32_t p = 0x80000000u, sq = 0x00800000u;   // x^0, x^8
    while (nbytes) {
        if (nbytes & 1u) p = crc_mul(sq, p);
        sq = crc_mul(sq, sq);
        nbytes >>= 1;
    }
    return crc_mul(p, crc);
}

__host__ __device__ inline uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ CRC_POLY : i >> 1;
    return i;
}

}  // namespace sarlacc
