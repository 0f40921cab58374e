// links_verify_core.hpp -- the banded unit-cost distance of one pair of reads (DESIGN §4.19 rule 6a), as the per-lane body
// of k_links_verify (links_verify.hip).  It compiles for the host as well, so that a stand-alone program can hold it to a
// plain DP under the host's sanitizers.
//
// The technique is k_msa_pairwise_bv's (msa_pairwise.hip) without its records: Myers' bit-vector recurrence in Hyyro's
// form over the band's rows, which slide down one row per column.
//   * Column j holds the rows i = j - w .. j + w as vertical deltas (Pv: +1, Mv: -1) in the top B = 2 w + 1 bits of NW
//     32-bit words: bit 32 NW - 1 is always the band's bottom row, so the base that enters the band and its delta go in
//     at a fixed bit; the band's top row is bit OFF = 32 NW - B, the same for every pair of a launch.
//   * A cell outside the band is infinite in the rule.  One below the bottom edge is emulated by a vertical delta +1, one
//     above the top edge by a horizontal delta +1: the step from either then costs diagonal + 2, which never beats the
//     diagonal step (at most diagonal + 1), so every cell inside the band has the rule's value.  Rows above row 0 carry
//     D(i, j) = j - i (vertical -1, horizontal +1), which the recurrence keeps and which leaves D(0, j) = j.
//   * The walk starts w columns before the matrix, where the band holds rows -2 w .. 0 only: w steps that slide the rows
//     1 .. w in (D(i, 0) = i is the bottom edge's +1) replace a loop that would set column 0 bit by bit.
//   * The distance is followed on the diagonal of the final cell: it starts at ||x| - |y|| and grows by one in every
//     column whose diagonal delta there is 1.  It never shrinks, so a pair is decided as soon as it passes `limit`.
//   * Bases come in 8-byte grabs, eight columns ahead of their use; a grab touches no byte outside its read.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define LV_FN __host__ __device__ __forceinline__
#else
#define LV_FN inline
#endif

namespace sarlacc {

constexpr int LV_MAX_BANDWIDTH = 127;
constexpr long long LV_PPM = 1000000;

// words of a band of 2 w + 1 bits, among those the kernel is built for: 1, 2, 4, 7 (the default w = 100), 8
constexpr int lv_words(int w) { return w <= 15 ? 1 : w <= 31 ? 2 : w <= 63 ? 4 : w <= 111 ? 7 : 8; }

// the low word of (hi : lo) >> 1
LV_FN uint32_t lv_slide(uint32_t hi, uint32_t lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, 1);
#else
    return (lo >> 1) | (hi << 31);
#endif
}

// rule 1: A 0, C 1, G 2, T 3 in upper case, every other byte 4; no branch
LV_FN uint32_t lv_code(uint32_t b) {
    const uint32_t x = (b >> 1) & 3u, c = x ^ (x >> 1);
    return ((0x54474341u >> (8 * c)) & 0xffu) == b ? c : 4u;
}

// bytes p .. p + 7 of a read of len bytes, byte e in bits 8 e .. 8 e + 7; 0 (no base) where p + e lies outside the read
LV_FN uint64_t lv_grab(const uint8_t* s, int p, int len) {
    uint64_t v = 0;
    if (p >= 0 && p <= len - 8) {
        std::memcpy(&v, s + p, 8);
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int e = 0; e < 8; ++e)
            if (p + e >= 0 && p + e < len) v |= static_cast<uint64_t>(s[p + e]) << (8 * e);
    }
    return v;
}

// D_w(x, y) of rule 6a, or with rev D_w(x, rc(y)), for ||x| - |y|| <= w <= 16 NW - 1; any value above `limit` stands for
// every distance above it.  y is read from its end for rc, the complement taken in the code.
template <int NW>
LV_FN int lv_banded(const uint8_t* x, int lx, const uint8_t* y, int ly, int w, bool rev, int limit) {
    const int OFF = 32 * NW - (2 * w + 1);
    uint32_t Pv[NW], Mv[NW], R0[NW], R1[NW], R2[NW];      // R2: the row is no base
    uint32_t inb[NW], top[NW], fin[NW];                    // the band's bits, its top row, the final cell's diagonal
    const int pbit = OFF + w + lx - ly;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < NW; ++k) {
        const int below = OFF - 32 * k;                    // bits of this word under the band
        inb[k] = below <= 0 ? ~0u : (below >= 32 ? 0u : ~((1u << below) - 1u));
        top[k] = (below >= 0 && below < 32) ? (1u << below) : 0u;
        fin[k] = (pbit >> 5) == k ? (1u << (pbit & 31)) : 0u;
        Pv[k] = 0u; Mv[k] = inb[k];
        R0[k] = R1[k] = 0u; R2[k] = ~0u;
    }
    int dist = lx > ly ? lx - ly : ly - lx;
    uint64_t rcur = 0, rnext = lv_grab(x, 0, lx), ccur = 0, cnext = lv_grab(y, rev ? ly - 8 : 0, ly);
    // step s slides row s in; from s = w + 1 on it also computes column j = s - w
    for (int s = 1; s <= w + ly && dist <= limit; ++s) {
        const int er = (s - 1) & 7;
        if (er == 0) { rcur = rnext; rnext = lv_grab(x, s + 7, lx); }
        const uint32_t cn = lv_code(static_cast<uint32_t>(rcur >> (8 * er)) & 0xffu);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < NW; ++k) {
            const bool last = k == NW - 1;
            const int up = last ? k : k + 1;
            Pv[k] = last ? ((Pv[k] >> 1) | 0x80000000u) : lv_slide(Pv[up], Pv[k]);
            Mv[k] = last ? (Mv[k] >> 1) : lv_slide(Mv[up], Mv[k]);
            R0[k] = last ? ((R0[k] >> 1) | ((cn & 1u) << 31)) : lv_slide(R0[up], R0[k]);
            R1[k] = last ? ((R1[k] >> 1) | (((cn >> 1) & 1u) << 31)) : lv_slide(R1[up], R1[k]);
            R2[k] = last ? ((R2[k] >> 1) | ((cn >> 2) << 31)) : lv_slide(R2[up], R2[k]);
        }
        const int j = s - w;
        if (j < 1) continue;
        const int ec = (j - 1) & 7;
        if (ec == 0) { ccur = cnext; cnext = lv_grab(y, rev ? ly - j - 15 : j + 7, ly); }
        uint32_t cc = lv_code(static_cast<uint32_t>(ccur >> (8 * (rev ? 7 - ec : ec))) & 0xffu);
        if (rev) cc ^= cc < 4u ? 3u : 0u;
        const uint32_t m0 = 0u - (cc & 1u), m1 = 0u - ((cc >> 1) & 1u), mx = 0u - (cc >> 2);      // mx: the column is no base
        uint32_t carry = 0u, ph_in = 0u, mh_in = 0u, grew = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < NW; ++k) {
            const uint32_t Eq = ~((R0[k] ^ m0) | (R1[k] ^ m1) | R2[k] | mx);
            const uint32_t pv = Pv[k] & inb[k];           // rows that slid out through the top edge no longer count
            const uint64_t sum = static_cast<uint64_t>(Eq & pv) + pv + carry;
            carry = static_cast<uint32_t>(sum >> 32);
            const uint32_t Xh = (static_cast<uint32_t>(sum) ^ pv) | Eq;
            const uint32_t Xv = Eq | Mv[k];
            const uint32_t Ph = Mv[k] | ~(Xh | pv);
            const uint32_t Mh = pv & Xh;
            grew |= ~(Xh | Mv[k]) & fin[k];               // the diagonal delta on the final cell's diagonal
            const uint32_t Phs = (Ph << 1) | ph_in | top[k];
            const uint32_t Mhs = (Mh << 1) | mh_in;       // Mh is zero under the band: nothing enters at the edge
            ph_in = Ph >> 31; mh_in = Mh >> 31;
            Pv[k] = Mhs | ~(Xv | Phs);
            Mv[k] = Phs & Xv;
        }
        dist += grew ? 1 : 0;
    }
    return dist;
}

// rule 6a.3: the largest distance that passes, from max_diff_ppm and the longer read
LV_FN int lv_threshold(long long max_diff_ppm, int la, int lb) {
    return static_cast<int>(max_diff_ppm * (la > lb ? la : lb) / LV_PPM);
}

}  // namespace sarlacc
