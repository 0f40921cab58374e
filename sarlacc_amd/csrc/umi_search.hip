// umi_search.hip -- encoding and the thresholded neighbour search of the UMI stage on gfx950.
// Replaces sorted_trie (the reference's src/sorted_trie.cpp:107-278).  The trie returns exactly { j : d2(i,j) <= 2*limit } listed in the order A<C<G<T<N, shorter prefix first, ties by
// input index (SURVEY App.B Q11).  We get the same lists from an all-pairs tile kernel over the UMIs sorted in that
// order: 2-bit packed bases + N bit-mask per UMI, one thread per (row, tile), columns broadcast from LDS, a
// composition / length lower bound rejecting most pairs, then an exact banded DP in registers (band = limit, costs x2
// as in src/sorted_trie.cpp:13-21).  Only the upper triangle is evaluated.  Thresholds 1 to 3 on large sets take the
// split-key search below instead.  This file: the kernels and the device steps that enqueue them; which of them a call
// runs is decided in umi_host.cpp (plan_search, pair_edges).  Design: DESIGN.md "UMI stage".
#include "umi_common.hpp"

namespace sarlacc {

// ---------------------------------------------------------------------------
// encoding

// trie child order A,C,G,T,N (src/sorted_trie.cpp:10); a character outside ACGTN counts as N and sets bad[0] to the
// smallest string index s that holds one
__device__ __forceinline__ unsigned umi_base(uint8_t c, int s, int* bad) {
    switch (c) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        case 'N': return 4;
        default: atomicMin(&bad[0], s); return 4;
    }
}

// members: optional 1-based ids selecting the strings of one pre-group.
__global__ void k_umi_encode(const uint8_t* chars, const int64_t* off, const int32_t* members, int n,
                             UmiArrays U, unsigned long long* key_hi, unsigned long long* key_lo, int* idx,
                             const uint8_t* skip /* optional: elements that are never compared (pre-groups of one read pass
                                                    through unchecked, src/umi_group.cpp:39-42): encoded as empty strings */,
                             int* bad /* [0]: min local index with unsupported char, [1]: min index too long,
                                         [2]: max(-length) of the too long ones, i.e. minus the longest */) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const long long id = members ? static_cast<long long>(members[s]) - 1 : s;
    const long long o = off[id];
    const int len = (skip && skip[s]) ? 0 : static_cast<int>(min(off[id + 1] - o, static_cast<int64_t>(1 << 30)));
    idx[s] = s;
    if (len > UMI_MAXLEN) {
        atomicMin(&bad[1], s);
        atomicMin(&bad[2], -len);
        U.code[s] = 0; U.nmask[s] = 0; U.comp[s] = 0; U.meta[s] = 0; key_hi[s] = 0; key_lo[s] = 0;
        return;
    }
    unsigned long long code = 0, khi = 0, klo = 0;
    uint32_t nmask = 0, comp = 0;
    for (int i = 0; i < len; ++i) {
        const unsigned v = umi_base(chars[o + i], s, bad);
        if (v == 4) nmask |= 1u << i;
        else { code |= static_cast<unsigned long long>(v) << (2 * i); comp += 1u << (8 * v); }
        const unsigned long long k = v + 1;  // 0 = past the end, so prefixes sort first
        if (i < 21) khi |= k << (3 * (20 - i));
        else klo |= k << (3 * (20 - (i - 21)));
    }
    U.code[s] = code; U.nmask[s] = nmask; U.comp[s] = comp;
    U.meta[s] = static_cast<uint32_t>(len) | (static_cast<uint32_t>(__popc(nmask)) << 12);
    key_hi[s] = khi; key_lo[s] = klo;
}

// The same for strings of up to UMI_LONG_MAX bases: UMI_LONG_WORDS code / mask words, one sort key per 21 bases.
__global__ void k_umi_encode_long(const uint8_t* chars, const int64_t* off, const int32_t* members, int n,
                                  UmiArrays U, unsigned long long* keys /* [nkeys][n] */, int* idx,
                                  const uint8_t* skip, int* bad, int words, int nkeys) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const long long id = members ? static_cast<long long>(members[s]) - 1 : s;
    const long long o = off[id];
    const int len = (skip && skip[s]) ? 0 : static_cast<int>(off[id + 1] - o);   // <= 32 words: checked by the caller
    idx[s] = s;
    uint32_t comp = 0;
    int nN = 0;
    for (int w = 0; w < words; ++w) {
        unsigned long long code = 0;
        uint32_t nmask = 0;
        const int hi = min(len - 32 * w, 32);
        for (int i = 0; i < hi; ++i) {
            const unsigned v = umi_base(chars[o + 32 * w + i], s, bad);
            if (v == 4) { nmask |= 1u << i; ++nN; }
            else { code |= static_cast<unsigned long long>(v) << (2 * i); comp += 1u << (8 * v); }
        }
        U.code[w * U.stride + s] = code;
        U.nmask[w * U.stride + s] = nmask;
    }
    for (int k = 0; k < nkeys; ++k) {
        unsigned long long key = 0;
        const int hi = min(len - UMI_KEY_BASES * k, UMI_KEY_BASES);
        for (int i = 0; i < hi; ++i) {
            const uint8_t c = chars[o + UMI_KEY_BASES * k + i];
            const unsigned long long v = c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : c == 'T' ? 4 : 5;
            key |= v << (3 * (UMI_KEY_BASES - 1 - i));
        }
        keys[static_cast<long long>(k) * n + s] = key;
    }
    U.comp[s] = words > UMI_LONG_WORDS ? 0u : comp;   // byte counters: at most 128 per letter (beyond 4 words the composition bound is not used)
    U.meta[s] = static_cast<uint32_t>(len) | (static_cast<uint32_t>(nN) << 12);
}

__global__ void k_gather_u64(const unsigned long long* src, const int* perm, unsigned long long* dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

__global__ void k_gather_gid(const int* gid, const int* perm, unsigned long long* key, int* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = gid[perm[i]];
    if (key) key[i] = static_cast<unsigned long long>(g);
    if (out) out[i] = g;
}

__global__ void k_gather_umi(UmiArrays src, const int* perm, UmiArrays dst, int n, int words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = perm[i];
    for (int w = 0; w < words; ++w) {
        dst.code[w * dst.stride + i] = src.code[w * src.stride + p];
        dst.nmask[w * dst.stride + i] = src.nmask[w * src.stride + p];
    }
    dst.comp[i] = src.comp[p]; dst.meta[i] = src.meta[p];
}

struct TileInfo;
struct PairArgs {
    UmiArrays U;                    // in (pre-group, trie) order
    const int* gid;                 // pre-group of every element in that order (nullptr: one group)
    int n;
    int lim2;
    unsigned long long* edges;      // (rank_i << 32 | rank_j), rank_i < rank_j
    unsigned long long* count;
    unsigned long long cap;
    int tile_lo;                    // first row tile of this launch (row tiles shard across GPUs)
    const uint32_t* tile_list;      // optional: the (row tile << 16 | column tile) pairs to search, one per block
    const TileInfo* sub_info;       // optional: common prefixes of the 64-element blocks (4 per tile)
    unsigned list_stride;           // block b searches tile_list[b * list_stride] (1; larger: a sample of the list)
    int special_lreq;               // >= 0: only pairs with a member that holds an N or is shorter than this (the rest
                                    // comes from the split-key search); -1: every pair
};

// ---------------------------------------------------------------------------
// Tile-level prefilter.  Inside a pre-group the elements are in trie (lexicographic) order, so
// the 256 strings of a tile share the common prefix of its first and last element.  A pair
// (s in row tile, t in column tile) within `L` edits aligns s[0..m) with some t[0..m'),
// |m - m'| <= L, at a cost <= L; with m <= |P_R| and m + L <= |P_C| both prefixes are known from
// the tiles alone, so whole tile pairs are discarded when no such m' exists -- exactly, because
// only pairs that cannot be neighbours are skipped.  Tiles that hold an N (a masked base costs
// half an edit) or span two pre-groups carry no prefix and are never discarded.
struct TileInfo {
    unsigned long long pcode;   // common prefix, 2 bits per base from bit 0
    int plen;                   // its length; -1: no information
    int special;                // some string of the tile holds an N or is shorter than `lreq`
};

template <int BLK>
__global__ void __launch_bounds__(BLK) k_tile_info(UmiArrays U, const int* gid, int n, int lreq, TileInfo* info) {
    const int t0 = blockIdx.x * BLK, t1 = min(t0 + BLK, n) - 1;
    const int i = t0 + threadIdx.x;
    const uint32_t nm = i < n ? U.nmask[i] : 0u;
    const int anyN = __syncthreads_or(nm != 0u);
    const int anyShort = __syncthreads_or(i < n && umi_len(U.meta[i]) < lreq);
    if (threadIdx.x != 0) return;
    TileInfo ti{0ull, -1, (anyN || anyShort) ? 1 : 0};
    if (!anyN && (!gid || gid[t0] == gid[t1])) {
        const unsigned long long a = U.code[t0], b = U.code[t1];
        const int la = umi_len(U.meta[t0]), lb = umi_len(U.meta[t1]);
        const unsigned long long x = a ^ b;
        int cp = x ? (__builtin_ctzll(x) >> 1) : 32;
        cp = min(cp, min(la, lb));
        ti.plen = cp;
        ti.pcode = cp >= 32 ? a : (a & ((1ull << (2 * cp)) - 1ull));
    }
    info[blockIdx.x] = ti;
}

// min over m' in [m - L, m + L] of the edit distance between x[0..m) and y[0..m') (unit costs),
// y known to at least m + L bases; > L is reported as L + 1.
template <int L>
__device__ __forceinline__ int prefix_dist(unsigned long long x, int m, unsigned long long y) {
    constexpr int BW = 2 * L + 1;
    int v[BW];   // v[d]: D[i][i + d - L]
#pragma unroll
    for (int d = 0; d < BW; ++d) v[d] = (d >= L) ? d - L : (L + 1);   // row 0: D[0][j] = j
    for (int i = 1; i <= m; ++i) {
        const unsigned xi = static_cast<unsigned>(x >> (2 * (i - 1))) & 3u;
        int left = L + 1;
#pragma unroll
        for (int d = 0; d < BW; ++d) {
            const int j = i + d - L;
            int best = L + 1;
            if (j == 0) best = i;
            else if (j > 0) {
                const unsigned yj = static_cast<unsigned>(y >> (2 * (j - 1))) & 3u;
                best = v[d] + (xi == yj ? 0 : 1);                 // D[i-1][j-1]
                if (d + 1 < BW) best = min(best, v[d + 1] + 1);   // D[i-1][j]
                best = min(best, left + 1);                        // D[i][j-1]
            }
            best = min(best, L + 1);
            v[d] = best;
            left = best;
        }
    }
    int res = L + 1;
#pragma unroll
    for (int d = 0; d < BW; ++d) res = min(res, v[d]);
    return res;
}

template <int L>
__global__ void k_tile_pairs(const TileInfo* info, int nt, int tile_lo, int tile_hi, int special_only, uint32_t* list, unsigned int* count) {
    const int bj = blockIdx.x * blockDim.x + threadIdx.x;
    const int bi = blockIdx.y + tile_lo;
    if (bi >= tile_hi || bj >= nt || bj < bi) return;
    bool keep = true;
    if (special_only && !info[bi].special && !info[bj].special) keep = false;
    if (keep && bj != bi) {
        const TileInfo R = info[bi], C = info[bj];
        if (R.plen >= 0 && C.plen >= 0) {
            // either orientation may prove that the tiles hold no neighbours
            const int m1 = min(R.plen, C.plen - L), m2 = min(C.plen, R.plen - L);
            if (m1 > L && prefix_dist<L>(R.pcode, m1, C.pcode) > L) keep = false;
            if (keep && m2 > L && prefix_dist<L>(C.pcode, m2, R.pcode) > L) keep = false;
        }
    }
    if (keep) list[atomicAdd(count, 1u)] = (static_cast<uint32_t>(bi) << 16) | static_cast<uint32_t>(bj);
}

// Shifted-Hamming lower bound for N-free pairs: a position of `a` that differs from b at every
// shift -K..K cannot be matched by any alignment within the band, so it costs a substitution or
// an indel (2 each).  More than `limit` such positions => d2 > 2*limit.
template <int K>
__device__ __forceinline__ bool shd_reject(unsigned long long ca, int la, unsigned long long cb, int lb, int limit) {
    const unsigned long long EVEN = 0x5555555555555555ull;
    const unsigned long long amask = la >= 32 ? ~0ull : ((1ull << (2 * la)) - 1ull);
    unsigned long long all = EVEN & amask;
#pragma unroll
    for (int s = -K; s <= K; ++s) {
        const unsigned long long xb = s >= 0 ? (cb >> (2 * s)) : (cb << (-2 * s));
        const unsigned long long diff = ca ^ xb;
        unsigned long long m = (diff | (diff >> 1)) & EVEN;
        // positions whose partner p+s falls outside b count as mismatches
        const int hi = lb - s;  // p < hi
        unsigned long long valid = hi >= 32 ? ~0ull : (hi <= 0 ? 0ull : ((1ull << (2 * hi)) - 1ull));
        if (s < 0) valid &= ~((1ull << (-2 * s)) - 1ull);
        m |= ~valid;
        all &= m;
    }
    return __popcll(all) > limit;
}

template <int K>
__global__ void __launch_bounds__(TILE) k_umi_pairs(const PairArgs A) {
    int bi = blockIdx.x + A.tile_lo, bj = blockIdx.y;
    if (A.tile_list) { const uint32_t e = A.tile_list[static_cast<size_t>(blockIdx.x) * A.list_stride]; bi = static_cast<int>(e >> 16); bj = static_cast<int>(e & 0xffffu); }
    if (bj < bi) return;
    // column tile (c*) and row tile (r*) both live in LDS: survivors of the cheap filters are
    // queued per wave and evaluated 64 at a time, so the exact DP always runs on full waves
    __shared__ unsigned long long c_code[TILE], r_code[TILE];
    __shared__ uint32_t c_nmask[TILE], c_meta[TILE], r_nmask[TILE], r_meta[TILE];
    __shared__ uint4 c_key[TILE];  // {pre-group, meta, composition, N mask}: one broadcast read per column
    __shared__ uint32_t s_q1[TILE / 64][128], s_q2[TILE / 64][128];
    const int t = threadIdx.x;
    const int lane = t & 63, wv = t >> 6;
    if (A.gid && bj > bi) {
        // elements are sorted by pre-group: the tiles share no group unless the first group of
        // the column tile is still open at the end of the row tile
        const int row_last = min(bi * TILE + TILE, A.n) - 1;
        if (A.gid[bj * TILE] > A.gid[row_last]) return;
    }
    const int jcol = bj * TILE + t;
    if (jcol < A.n) {
        c_code[t] = A.U.code[jcol]; c_nmask[t] = A.U.nmask[jcol]; c_meta[t] = A.U.meta[jcol];
        c_key[t] = make_uint4(A.gid ? static_cast<uint32_t>(A.gid[jcol]) : 0u, A.U.meta[jcol], A.U.comp[jcol], A.U.nmask[jcol]);
    } else {
        c_code[t] = 0; c_nmask[t] = 0; c_meta[t] = UMI_META_NONE;  // never matches
        c_key[t] = make_uint4(0xffffffffu, UMI_META_NONE, 0u, 0u);
    }
    const int i = bi * TILE + t;
    const bool row_on = i < A.n;
    const unsigned long long ca = row_on ? A.U.code[i] : 0ull;
    const uint32_t na = row_on ? A.U.nmask[i] : 0u, compa = row_on ? A.U.comp[i] : 0u, ma = row_on ? A.U.meta[i] : UMI_META_NONE;
    r_code[t] = ca; r_nmask[t] = na; r_meta[t] = ma;
    __syncthreads();
    const int la = umi_len(ma), nNa = umi_nn(ma);
    const int gi = (row_on && A.gid) ? A.gid[i] : (row_on ? 0 : -2);
    const int limit = A.lim2 / 2;
    const bool row_special = A.special_lreq < 0 || na != 0u || la < A.special_lreq;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t* const q1 = s_q1[wv];   // pairs that passed the length / composition bounds
    uint32_t* const q2 = s_q2[wv];   // ... and the shifted-Hamming bound: exact DP pending
    int n1 = 0, n2 = 0;              // wave-uniform fill levels

    // Two-level compaction: each filter runs on full waves of candidates, so a rare survivor
    // never drags 63 idle lanes through the next, more expensive stage.
    auto run_dp = [&](int count) {
        if (lane < count) {
            const uint32_t e = q2[lane];
            const int ti = e >> 8, jj = e & 0xff;
            const uint32_t mra = r_meta[ti], mcb = c_meta[jj];
            const int d = banded_lev2<K>(WordStr{r_code[ti], r_nmask[ti]}, umi_len(mra), WordStr{c_code[jj], c_nmask[jj]}, umi_len(mcb), A.lim2);
            if (d <= A.lim2) {
                const unsigned long long slot = atomicAdd(A.count, 1ull);
                if (slot < A.cap)
                    A.edges[slot] = (static_cast<unsigned long long>(bi * TILE + ti) << 32) | static_cast<unsigned>(bj * TILE + jj);
            }
        }
    };
    auto push2 = [&](bool keep, uint32_t e) {
        const unsigned long long m = __ballot(keep);
        if (m) {
            if (keep) q2[n2 + __popcll(m & lt)] = e;
            n2 += __popcll(m);
            if (n2 >= 64) {
                run_dp(64);
                const uint32_t moved = (64 + lane < n2) ? q2[64 + lane] : 0u;
                if (64 + lane < n2) q2[lane] = moved;
                n2 -= 64;
            }
        }
    };
    auto run_shd = [&](int count) {
        bool keep = false;
        uint32_t e = 0;
        if (lane < count) {
            e = q1[lane];
            const int ti = e >> 8, jj = e & 0xff;
            keep = true;
            if (K <= 8 && (r_nmask[ti] | c_nmask[jj]) == 0u)
                keep = !shd_reject<(K <= 8 ? K : 0)>(r_code[ti], umi_len(r_meta[ti]), c_code[jj], umi_len(c_meta[jj]), limit);
        }
        push2(keep, e);
    };

    const int jn = min(TILE, A.n - bj * TILE);
    // Sub-tile prefilter: the 64 rows of this wave and each 64-column block of the tile have
    // longer common prefixes than the 256-element tiles; a block whose prefix cannot align with
    // the wave's within `limit` edits holds no neighbour of these rows (same argument as k_tile_pairs).
    unsigned sub_ok = 0xfu;
    if (K >= 1 && K <= 5 && A.sub_info && bi != bj) {
        bool ok = true;
        if (lane < 4) {
            const int rb = bi * 4 + wv, cb = bj * 4 + lane;
            if (rb * 64 < A.n && cb * 64 < A.n) {
                const TileInfo R = A.sub_info[rb], C = A.sub_info[cb];
                if (R.plen >= 0 && C.plen >= 0) {
                    constexpr int L = (K >= 1 && K <= 5) ? K : 1;
                    const int m1 = min(R.plen, C.plen - L), m2 = min(C.plen, R.plen - L);
                    if (m1 > L && prefix_dist<L>(R.pcode, m1, C.pcode) > L) ok = false;
                    if (ok && m2 > L && prefix_dist<L>(C.pcode, m2, R.pcode) > L) ok = false;
                }
            }
        }
        sub_ok = static_cast<unsigned>(__ballot(ok)) & 0xfu;
    }
    bool row_ok = true;   // this row can have neighbours in the current 64-column block
    for (int jj = 0; jj < jn; ++jj) {
        if (!((sub_ok >> (jj >> 6)) & 1u)) { jj |= 63; continue; }   // skip the whole 64-column block
        if (K >= 1 && K <= 3 && A.sub_info && bi != bj && (jj & 63) == 0) {
            // the row's own string is fully known: the block's whole prefix has to align with its
            // first plen +- limit bases within `limit` edits
            constexpr int L = (K >= 1 && K <= 3) ? K : 1;
            const TileInfo C = A.sub_info[bj * 4 + (jj >> 6)];
            const int m2 = min(C.plen, la - L);
            row_ok = !(row_on && na == 0u && C.plen >= 0 && m2 > L && prefix_dist<L>(C.pcode, m2, ca) > L);
            if (!__ballot(row_ok)) { jj |= 63; continue; }
        }
        const uint4 ck = c_key[jj];
        bool pass = row_ok && row_on && static_cast<int>(ck.x) == gi && (bi != bj || jj > t);
        {
            const int lb = umi_len(ck.y), nNb = umi_nn(ck.y);
            const int dl = la > lb ? la - lb : lb - la;
            // composition lower bound: every edit costs >= 1 and moves the 5-letter composition by
            // <= 2 (<= its cost when no N is involved)
            const int l1 = static_cast<int>(__builtin_amdgcn_sad_u8(compa, ck.z, 0u)) + (nNa > nNb ? nNa - nNb : nNb - nNa);
            const bool anyN = (na | ck.w) != 0u;
            pass = pass && 2 * dl <= A.lim2 && l1 <= (anyN ? 2 * A.lim2 : A.lim2);
            pass = pass && (row_special || ck.w != 0u || lb < A.special_lreq);
        }
        const unsigned long long mask = __ballot(pass);
        if (mask) {
            if (pass) q1[n1 + __popcll(mask & lt)] = (static_cast<uint32_t>(t) << 8) | static_cast<uint32_t>(jj);
            n1 += __popcll(mask);
            if (n1 >= 64) {
                run_shd(64);
                const uint32_t moved = (64 + lane < n1) ? q1[64 + lane] : 0u;
                if (64 + lane < n1) q1[lane] = moved;
                n1 -= 64;
            }
        }
    }
    run_shd(n1);
    run_dp(n2);
}

// ---------------------------------------------------------------------------
// Strings of 33..UMI_LONG_MAX bases (4-word codes).  Same distance, same tiling, the same exact
// length / composition bounds; the prefix and shifted-Hamming filters of the one-word path are not
// carried over (they are only filters: the result is the same set of pairs).

// K: band held in registers; K < 0: full DP.  XL: strings of more than UMI_LONG_MAX bases -- as many words as the longest
// needs (up to UMI_XL_WORDS), read where they lie in HBM instead of from a staged tile (the planes of a tile's 256 strings
// are 2 KB runs each; the words a band touches stay in L1 / L2), no composition bound (its byte counters stop at 255).
template <int K, bool XL>
__global__ void __launch_bounds__(TILE) k_umi_pairs_long(const PairArgs A) {
    const int bi = blockIdx.x + A.tile_lo, bj = blockIdx.y;
    if (bj < bi) return;
    constexpr int SW = XL ? 1 : UMI_LONG_WORDS;   // staged words per string
    __shared__ unsigned long long c_code[SW * TILE], r_code[SW * TILE];
    __shared__ uint32_t c_nmask[SW * TILE], r_nmask[SW * TILE];
    __shared__ uint4 c_key[TILE];  // {pre-group, meta, composition, any N}
    const int t = threadIdx.x;
    if (A.gid && bj > bi) {
        const int row_last = min(bi * TILE + TILE, A.n) - 1;
        if (A.gid[bj * TILE] > A.gid[row_last]) return;
    }
    const int jcol = bj * TILE + t, i = bi * TILE + t;
    const bool row_on = i < A.n;
    uint32_t anyN_col = 0, na = 0;
    if (XL) {   // only "some base is N" is needed up front
        anyN_col = (jcol < A.n && umi_nn(A.U.meta[jcol]) > 0) ? 1u : 0u;
        na = (row_on && umi_nn(A.U.meta[i]) > 0) ? 1u : 0u;
    } else {
        for (int w = 0; w < UMI_LONG_WORDS; ++w) {
            const bool on = jcol < A.n;
            c_code[w * TILE + t] = on ? A.U.code[w * A.U.stride + jcol] : 0ull;
            const uint32_t m = on ? A.U.nmask[w * A.U.stride + jcol] : 0u;
            c_nmask[w * TILE + t] = m;
            anyN_col |= m;
            r_code[w * TILE + t] = row_on ? A.U.code[w * A.U.stride + i] : 0ull;
            const uint32_t mr = row_on ? A.U.nmask[w * A.U.stride + i] : 0u;
            r_nmask[w * TILE + t] = mr;
            na |= mr;
        }
    }
    c_key[t] = jcol < A.n ? make_uint4(A.gid ? static_cast<uint32_t>(A.gid[jcol]) : 0u, A.U.meta[jcol], A.U.comp[jcol], anyN_col)
                          : make_uint4(0xffffffffu, UMI_META_NONE, 0u, 0u);
    __syncthreads();
    const uint32_t compa = row_on ? A.U.comp[i] : 0u, ma = row_on ? A.U.meta[i] : UMI_META_NONE;
    const int la = umi_len(ma), nNa = umi_nn(ma);
    const int gi = (row_on && A.gid) ? A.gid[i] : (row_on ? 0 : -2);
    const int gstride = static_cast<int>(A.U.stride);
    const LongStr sa = XL ? LongStr{A.U.code + (row_on ? i : 0), A.U.nmask + (row_on ? i : 0), gstride} : LongStr{r_code + t, r_nmask + t, TILE};
    const int jn = min(TILE, A.n - bj * TILE);
    for (int jj = 0; jj < jn; ++jj) {
        const uint4 ck = c_key[jj];
        bool pass = row_on && static_cast<int>(ck.x) == gi && (bi != bj || jj > t);
        const int lb = umi_len(ck.y), nNb = umi_nn(ck.y);
        const int dl = la > lb ? la - lb : lb - la;
        // the composition bound of k_umi_pairs; the byte counters hold up to 128 per letter, sad_u8 is exact
        const int l1 = static_cast<int>(__builtin_amdgcn_sad_u8(compa, ck.z, 0u)) + (nNa > nNb ? nNa - nNb : nNb - nNa);
        const bool anyN = (na | ck.w) != 0u;
        pass = pass && 2 * dl <= A.lim2 && l1 <= (anyN ? 2 * A.lim2 : A.lim2);
        if (!pass) continue;
        const LongStr sb = XL ? LongStr{A.U.code + bj * TILE + jj, A.U.nmask + bj * TILE + jj, gstride} : LongStr{c_code + jj, c_nmask + jj, TILE};
        int d;
        if constexpr (K >= 0) d = banded_lev2<(K >= 0 ? K : 0)>(sa, la, sb, lb, A.lim2);
        else d = full_lev2<(XL ? UMI_XL_MAX : UMI_LONG_MAX)>(sa, la, sb, lb, A.lim2);
        if (d <= A.lim2) {
            const unsigned long long slot = atomicAdd(A.count, 1ull);
            if (slot < A.cap)
                A.edges[slot] = (static_cast<unsigned long long>(bi * TILE + t) << 32) | static_cast<unsigned>(bj * TILE + jj);
        }
    }
}

// ---------------------------------------------------------------------------
// Split-key neighbour search for thresholds 1 to 3 on large sets.
//
// The all-tile-pairs search above looks at every pair: at threshold 3 on 12-base UMIs its length, composition and
// shifted-Hamming bounds pass most of them on to the exact DP.  The search below enumerates candidates instead.
// Let lev(a, b) <= k for N-free a, b, and fix h, s with h + s <= |a|.  An optimal alignment sends a[0..h) to a prefix
// b1 of b and the rest of a to the rest of b; the costs of the two parts sum to <= k.  So with k1 + k2 = k - 1
//     P(a,b): some prefix of b is within k1 edits of the first h bases of a,  or
//     S(a,b): some suffix of b is within k2 edits of the last s bases of a
// (the last s bases of a lie inside the second part, and the part of an alignment that covers them costs no more than
// the whole; threshold 1: k1 = k2 = 0, one of the two keys matches exactly).  With k1, k2 <= 1 the strings b that satisfy P(a, .) are those that start with one of the <= 8h + 5
// one-edit variants of a[0..h) -- a union of contiguous ranges of the set in trie order; S(a, .) the same in the order
// of the reversed strings.  Rows that share their first h bases share the ranges, so the work items are (row group,
// 256 candidate columns); a lane holds one column as the pattern of a bit-vector edit distance (Myers 1999 / Hyyro
// 2003, global variant) and the rows of the group stream through as the text, from scalar registers.
// Every pair {a, b} is reported once, from its lower-ranked member a: by the prefix scan if P(a, b), else by the
// suffix scan (which evaluates P(a, b) on the first h + 1 bases to leave those pairs to the prefix scan).  Only a
// needs h + s <= |a|, so the rows are scanned by length class, each with keys of half its length (at most 8 bases),
// against columns of any length.
// Strings with an N (a masked base costs half an edit: the argument above does not hold) or shorter than 8 bases are
// "special": their pairs come from the tile kernel restricted to pairs with a special member.
// The result is the same set of pairs as the tile search (tests: both against the oracle and against each other).

struct SkElem {
    uint32_t plo, phi;   // bit planes of the 2-bit codes, base i at bit i; the scan order's own orientation
    uint32_t meta;       // len | special << 6 | (first 9 bases of the FORWARD string, 2 bits each) << 8
    uint32_t rank;       // rank in trie order
};

__device__ __forceinline__ uint32_t sk_even_bits(unsigned long long x) {   // bits 0, 2, 4, ... of x -> bits 0, 1, 2, ...
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return static_cast<uint32_t>(x);
}

__device__ __forceinline__ unsigned long long sk_order_key(uint32_t plo, uint32_t phi, uint32_t nmask, int len) {
    unsigned long long k = 0;
    const int m = min(len, 21);
    for (int i = 0; i < m; ++i) {
        const unsigned long long d = ((nmask >> i) & 1u) ? 5ull : 1ull + ((plo >> i) & 1u) + 2ull * ((phi >> i) & 1u);
        k |= d << (3 * (20 - i));
    }
    return k;
}

__global__ void __launch_bounds__(256) k_sk_lenhist(UmiArrays U, int n, unsigned int* hist /* [34]: lengths 0..32, [33] strings with an N */) {
    __shared__ unsigned int s_h[34];
    if (threadIdx.x < 34) s_h[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        atomicAdd(&s_h[min(umi_len(U.meta[i]), 32)], 1u);
        if (U.nmask[i]) atomicAdd(&s_h[33], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 34 && s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// Elements in trie order (REV = false) or, per trie rank, the reversed string with its sort key (REV = true).
template <bool REV>
__global__ void k_sk_elems(UmiArrays U, int n, int lreq, SkElem* el, unsigned long long* okey, int* val) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long code = U.code[i];
    const uint32_t nm = U.nmask[i];
    const int len = umi_len(U.meta[i]);
    uint32_t plo = sk_even_bits(code), phi = sk_even_bits(code >> 1), nmo = nm;
    if (REV && len > 0) { plo = __brev(plo) >> (32 - len); phi = __brev(phi) >> (32 - len); nmo = __brev(nm) >> (32 - len); }
    const uint32_t special = (nm != 0u || len < lreq) ? 1u : 0u;
    el[i] = SkElem{plo, phi, static_cast<uint32_t>(len) | (special << 6) | (static_cast<uint32_t>(code & 0x3ffffull) << 8), static_cast<uint32_t>(i)};
    okey[i] = sk_order_key(plo, phi, nmo, len);
    if (REV) val[i] = i;
}

__global__ void k_sk_permute(const SkElem* el, const int* val, const int* gid, int n, SkElem* out, int* gid_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = val[i];
    out[i] = el[r];
    if (gid_out) gid_out[i] = gid[r];
}

// Row groups: maximal runs of the scan order that share pre-group and first h bases.
__global__ void k_sk_group_flags(SkOrder O, int h, int* flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > O.n) return;
    if (i == O.n) { flag[i] = 0; return; }
    bool f = i == 0;
    if (!f) {
        const int sh = 3 * (21 - h);
        f = (O.okey[i] >> sh) != (O.okey[i - 1] >> sh) || (O.gid && O.gid[i] != O.gid[i - 1]);
    }
    flag[i] = f ? 1 : 0;
}

__global__ void k_sk_group_starts(const int* flag, const long long* pos, int n, int* start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { start[pos[n]] = n; return; }
    if (flag[i]) start[pos[i]] = i;
}

constexpr int SK_MAXR = 72;    // ranges per row group: 1 + 3h + h + 4(h + 1) <= 69 for h <= 8
constexpr int SK_ROWS = 128;   // rows per work item
constexpr int SK_COLS = 256;   // candidate columns per work item (one per thread)

// first index of the scan order whose (pre-group, key) is >= (g, k) [upper = false] or > (g, k) [upper = true]
__device__ __forceinline__ int sk_bound(const SkOrder& O, int g, unsigned long long k, bool upper) {
    int lo = 0, hi = O.n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int gm = O.gid ? O.gid[mid] : 0;
        const unsigned long long km = O.okey[mid];
        const bool before = gm != g ? gm < g : (upper ? km <= k : km < k);
        if (before) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The candidate columns of every row group: ranges of the scan order that start with a variant (<= k1 edits) of the
// group's first h bases, merged, as (start, candidates before it); `clip`: columns from the group's own start on
// (trie order: a pair is reported from its lower-ranked member).
__global__ void k_sk_ranges(SkOrder O, const int* rg_start, int nrg, int h, int k1, int clip,
                            int2* ranges, int* nranges, int* ctotal, long long* items) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > nrg) return;
    if (g == nrg) { items[g] = 0; return; }
    const int r0 = rg_start[g], r1 = rg_start[g + 1];
    const unsigned long long key = O.okey[r0];
    const int grp = O.gid ? O.gid[r0] : 0;
    int d[10];
    bool plain = true;   // first h bases present and N-free
    for (int i = 0; i < h; ++i) { d[i] = static_cast<int>((key >> (3 * (20 - i))) & 7ull); plain = plain && d[i] >= 1 && d[i] <= 4; }
    int lo[SK_MAXR], hi[SK_MAXR], nr = 0;
    auto add = [&](const int* v, int m) {
        unsigned long long k = 0;
        for (int i = 0; i < m; ++i) k |= static_cast<unsigned long long>(v[i]) << (3 * (20 - i));
        const unsigned long long fill = (1ull << (3 * (21 - m))) - 1ull;
        int a = sk_bound(O, grp, k, false);
        const int b = sk_bound(O, grp, k | fill, true);
        if (clip) a = max(a, r0);
        if (a >= b) return;
        // insert by start
        int p = nr++;
        while (p > 0 && lo[p - 1] > a) { lo[p] = lo[p - 1]; hi[p] = hi[p - 1]; --p; }
        lo[p] = a; hi[p] = b;
    };
    if (plain) {
        int v[10];
        for (int i = 0; i < h; ++i) v[i] = d[i];
        add(v, h);
        if (k1 >= 1) {
            for (int p = 0; p < h; ++p) {           // substitutions
                for (int c = 1; c <= 4; ++c) if (c != d[p]) { v[p] = c; add(v, h); }
                v[p] = d[p];
            }
            for (int p = 0; p < h; ++p) {           // one base of the h missing in b
                if (p > 0 && d[p] == d[p - 1]) continue;   // the same string as deleting p - 1
                int m = 0;
                for (int i = 0; i < h; ++i) if (i != p) v[m++] = d[i];
                add(v, h - 1);
            }
            for (int p = 0; p <= h; ++p)            // one more base in b
                for (int c = 1; c <= 4; ++c) {
                    if (p < h && c == d[p]) continue;      // the same string as inserting after the run
                    int m = 0;
                    for (int i = 0; i < p; ++i) v[m++] = d[i];
                    v[m++] = c;
                    for (int i = p; i < h; ++i) v[m++] = d[i];
                    add(v, h + 1);
                }
        }
    }
    // merge overlapping ranges
    int out = 0, total = 0;
    int2* R = ranges + static_cast<long long>(g) * SK_MAXR;
    int ca = 0, cb = 0;
    for (int i = 0; i < nr; ++i) {
        if (i == 0) { ca = lo[0]; cb = hi[0]; continue; }
        if (lo[i] <= cb) { cb = max(cb, hi[i]); continue; }
        R[out++] = make_int2(ca, total); total += cb - ca;
        ca = lo[i]; cb = hi[i];
    }
    if (nr) { R[out++] = make_int2(ca, total); total += cb - ca; }
    nranges[g] = out;
    ctotal[g] = total;
    items[g] = static_cast<long long>((r1 - r0 + SK_ROWS - 1) / SK_ROWS) * ((total + SK_COLS - 1) / SK_COLS);
}

// P(x, y): some prefix of y (ly bases long) within k1 (0 or 1) edits of the first h bases of x; x, y: 2-bit codes of the
// first 9 bases (zero beyond the end) -- exactly "y starts with one of the variants k_sk_ranges lists for x".
__device__ __forceinline__ bool sk_prefix_within(uint32_t x, uint32_t y, int ly, int h, int k1) {
    auto mism = [](uint32_t u) { return (u | (u >> 1)) & 0x55555555u; };
    const uint32_t mh = (1u << (2 * h)) - 1u;
    const uint32_t d0 = mism(x ^ y) & mh;
    if (ly >= h && __popc(d0) <= k1) return true;
    if (k1 == 0 || ly < h - 1) return false;
    const int f = d0 ? (__builtin_ctz(d0) >> 1) : h;             // first mismatch
    const uint32_t d1 = mism((x >> 2) ^ y) & (mh >> 2);          // x[p + 1] against y[p], p < h - 1
    const uint32_t d2 = mism(x ^ (y >> 2)) & mh;                 // x[p] against y[p + 1], p < h
    if ((d1 >> (2 * min(f, h - 1))) == 0u) return true;          // x without its base p is a prefix of y
    return ly >= h + 1 && (d2 >> (2 * min(f, h))) == 0u;         // x with one base inserted at p is a prefix of y
}

struct SkScanArgs {
    const SkElem* el;
    const int* rg_start;
    int nrg;
    const int2* ranges;
    const int* nranges;
    const int* ctotal;
    const long long* item_off;     // [nrg + 1] exclusive
    unsigned item_stride;          // block b works on item b * item_stride (1; larger: a sample)
    int limit, h, k1;              // threshold; the prefix split (the suffix scan's check of P)
    int len_lo, len_hi;            // rows of this launch: lengths len_lo..len_hi (their keys are h and s bases long)
    uint32_t row_lo, row_hi;       // trie ranks of the rows this launch reports (row tiles shard across GPUs)
    unsigned long long* edges;
    unsigned long long* count;
    unsigned long long cap;
};

template <bool SUFFIX>
__global__ void __launch_bounds__(SK_COLS) k_sk_scan(const SkScanArgs A) {
    __shared__ int2 s_rng[SK_MAXR];
    __shared__ unsigned long long s_q[SK_COLS / 64][128];
    __shared__ SkElem s_rows[SK_ROWS];
    const int t = threadIdx.x, lane = t & 63;
    const long long item = static_cast<long long>(blockIdx.x) * A.item_stride;
    int g = 0;
    {
        int lo = 0, hi = A.nrg;   // item_off[lo] <= item < item_off[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.item_off[mid] <= item) lo = mid; else hi = mid; }
        g = lo;
    }
    const int r0g = A.rg_start[g], r1g = A.rg_start[g + 1];
    const int C = A.ctotal[g], ncc = (C + SK_COLS - 1) / SK_COLS;
    const long long local = item - A.item_off[g];
    const int rc = static_cast<int>(local / ncc), cc = static_cast<int>(local % ncc);
    const int r0 = r0g + rc * SK_ROWS, r1 = min(r0 + SK_ROWS, r1g);
    const int nr = A.nranges[g];
    if (t < nr) s_rng[t] = A.ranges[static_cast<long long>(g) * SK_MAXR + t];
    if (t < r1 - r0) s_rows[t] = A.el[r0 + t];
    __syncthreads();
    const int vc = cc * SK_COLS + t;
    int col = -1;
    if (vc < C) {
        int a = 0, b = nr;
        while (b - a > 1) { const int m = (a + b) >> 1; if (s_rng[m].y <= vc) a = m; else b = m; }
        col = s_rng[a].x + (vc - s_rng[a].y);
    }
    SkElem e{0u, 0u, 1u | (1u << 6), 0u};
    if (col >= 0) e = A.el[col];
    const int lb = e.meta & 63;
    const bool valid = col >= 0 && !((e.meta >> 6) & 1u);
    const int sh = 32 - (valid ? lb : 1);
    const uint32_t pl = e.plo << sh, ph = e.phi << sh, pat = ~0u << sh, low = (2u << sh) - 1u;
    const uint32_t cfwd = e.meta >> 8;
    unsigned long long* const q = s_q[t >> 6];
    const unsigned long long lt = (1ull << lane) - 1ull;
    int nq = 0;
    auto flush = [&](int count) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(A.count, static_cast<unsigned long long>(count));
        base = (static_cast<unsigned long long>(__shfl(static_cast<int>(base >> 32), 0)) << 32) | static_cast<unsigned>(__shfl(static_cast<int>(base), 0));
        if (lane < count && base + lane < A.cap) A.edges[base + lane] = q[lane];
    };
    for (int r = r0; r < r1; ++r) {
        const SkElem R = s_rows[r - r0];   // the same address in every lane: one broadcast read
        const uint32_t rmeta = __builtin_amdgcn_readfirstlane(R.meta);
        const uint32_t rrank = __builtin_amdgcn_readfirstlane(R.rank);
        const int la = rmeta & 63;
        if (((rmeta >> 6) & 1u) || la < A.len_lo || la > A.len_hi) continue;
        if (rrank < A.row_lo || rrank >= A.row_hi) continue;
        const uint32_t tlo = __builtin_amdgcn_readfirstlane(R.plo), thi = __builtin_amdgcn_readfirstlane(R.phi);
        uint32_t Pv = pat, Mv = 0u;
        for (int j = 0; j < la; ++j) {
            const uint32_t m0 = 0u - ((tlo >> j) & 1u), m1 = 0u - ((thi >> j) & 1u);
            const uint32_t Eq = ~((pl ^ m0) | (ph ^ m1)) & pat;
            const uint32_t Xv = Eq | Mv;
            const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
            uint32_t Ph = Mv | ~(Xh | Pv);
            uint32_t Mh = Pv & Xh;
            Ph = (Ph << 1) | low;
            Mh <<= 1;
            Pv = Mh | ~(Xv | Ph);
            Mv = Ph & Xv;
        }
        // D[lb][la] = D[0][la] + the vertical deltas down the last column (row 0 of a global alignment holds j)
        const int d = la + __popc(Pv & pat) - __popc(Mv & pat);
        bool hit = valid && d <= A.limit && e.rank > rrank;   // a pair is reported from its lower-ranked member
        if (SUFFIX) hit = hit && !sk_prefix_within(rmeta >> 8, cfwd, lb, A.h, A.k1);
        const unsigned long long ball = __ballot(hit);
        if (ball) {
            if (hit) q[nq + __popcll(ball & lt)] = (static_cast<unsigned long long>(rrank) << 32) | e.rank;
            nq += __popcll(ball);
            if (nq >= 64) {
                flush(64);
                const unsigned long long moved = (64 + lane < nq) ? q[64 + lane] : 0ull;
                if (64 + lane < nq) q[lane] = moved;
                nq -= 64;
            }
        }
    }
    if (nq) flush(nq);
}

// The same scan with TWO candidate columns per lane, for the rows of up to 15 - limit bases (12-base UMIs; a string of 16
// and more bases is no neighbour of such a row whatever it holds, so those columns are not valid here):
// the two patterns sit top-aligned in the halves of one 32-bit word, so every operation of the recurrence advances both.
// What crosses from the lower half into the upper one lands on bits below the upper pattern: the carry of the addition
// (bit 16 holds no pattern bit as long as the upper string has at most 15 bases, and nothing is added there, so it goes no
// further), the top bit of Ph << 1 (overwritten by `low`, the row-0 deltas) and the top bit of Mh << 1 (masked out).
// Work items, candidate ranges and the pairs reported are those of k_sk_scan; half the threads per item.
template <bool SUFFIX>
__global__ void __launch_bounds__(SK_COLS / 2) k_sk_scan_pk(const SkScanArgs A) {
    __shared__ int2 s_rng[SK_MAXR];
    __shared__ unsigned long long s_q[SK_COLS / 128][192];
    __shared__ SkElem s_rows[SK_ROWS];
    const int t = threadIdx.x, lane = t & 63;
    const long long item = static_cast<long long>(blockIdx.x) * A.item_stride;
    int g = 0;
    {
        int lo = 0, hi = A.nrg;   // item_off[lo] <= item < item_off[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.item_off[mid] <= item) lo = mid; else hi = mid; }
        g = lo;
    }
    const int r0g = A.rg_start[g], r1g = A.rg_start[g + 1];
    const int C = A.ctotal[g], ncc = (C + SK_COLS - 1) / SK_COLS;
    const long long local = item - A.item_off[g];
    const int rc = static_cast<int>(local / ncc), cc = static_cast<int>(local % ncc);
    const int r0 = r0g + rc * SK_ROWS, r1 = min(r0 + SK_ROWS, r1g);
    const int nr = A.nranges[g];
    if (t < nr) s_rng[t] = A.ranges[static_cast<long long>(g) * SK_MAXR + t];
    for (int q = t; q < r1 - r0; q += SK_COLS / 2) s_rows[q] = A.el[r0 + q];
    __syncthreads();
    auto column = [&](int vc) -> int {
        if (vc >= C) return -1;
        int a = 0, b = nr;
        while (b - a > 1) { const int m = (a + b) >> 1; if (s_rng[m].y <= vc) a = m; else b = m; }
        return s_rng[a].x + (vc - s_rng[a].y);
    };
    const int col0 = column(cc * SK_COLS + t), col1 = column(cc * SK_COLS + SK_COLS / 2 + t);
    const SkElem none{0u, 0u, 1u | (1u << 6), 0u};
    const SkElem e0 = col0 >= 0 ? A.el[col0] : none, e1 = col1 >= 0 ? A.el[col1] : none;
    const int lb0 = e0.meta & 63, lb1 = e1.meta & 63;
    const bool valid0 = col0 >= 0 && !((e0.meta >> 6) & 1u) && lb0 < 16, valid1 = col1 >= 0 && !((e1.meta >> 6) & 1u) && lb1 < 16;
    const int sh0 = 16 - (valid0 ? lb0 : 1), sh1 = 16 - (valid1 ? lb1 : 1);
    const uint32_t F = 0xFFFFu;
    const uint32_t pl = ((e0.plo << sh0) & F) | (((e1.plo << sh1) & F) << 16), ph = ((e0.phi << sh0) & F) | (((e1.phi << sh1) & F) << 16);
    const uint32_t pat = ((F << sh0) & F) | (((F << sh1) & F) << 16);
    const uint32_t low = ((2u << sh0) - 1u) | (((2u << sh1) - 1u) << 16), keep = ~low;
    const uint32_t cfwd0 = e0.meta >> 8, cfwd1 = e1.meta >> 8;
    unsigned long long* const q = s_q[t >> 6];
    const unsigned long long lt = (1ull << lane) - 1ull;
    int nq = 0;
    auto flush = [&](int count) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(A.count, static_cast<unsigned long long>(count));
        base = (static_cast<unsigned long long>(__shfl(static_cast<int>(base >> 32), 0)) << 32) | static_cast<unsigned>(__shfl(static_cast<int>(base), 0));
        if (lane < count && base + lane < A.cap) A.edges[base + lane] = q[lane];
    };
    for (int r = r0; r < r1; ++r) {
        const SkElem R = s_rows[r - r0];   // the same address in every lane: one broadcast read
        const uint32_t rmeta = __builtin_amdgcn_readfirstlane(R.meta);
        const uint32_t rrank = __builtin_amdgcn_readfirstlane(R.rank);
        const int la = rmeta & 63;
        if (((rmeta >> 6) & 1u) || la < A.len_lo || la > A.len_hi) continue;
        if (rrank < A.row_lo || rrank >= A.row_hi) continue;
        const uint32_t tlo = __builtin_amdgcn_readfirstlane(R.plo), thi = __builtin_amdgcn_readfirstlane(R.phi);
        uint32_t Pv = pat, Mv = 0u;
        for (int j = 0; j < la; ++j) {
            const uint32_t m0 = 0u - ((tlo >> j) & 1u), m1 = 0u - ((thi >> j) & 1u);
            const uint32_t Eq = ~((pl ^ m0) | (ph ^ m1)) & pat;
            const uint32_t Xv = Eq | Mv;
            const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
            uint32_t Ph = Mv | ~(Xh | Pv);
            uint32_t Mh = Pv & Xh;
            Ph = (Ph << 1) | low;
            Mh = (Mh << 1) & keep;
            Pv = Mh | ~(Xv | Ph);
            Mv = Ph & Xv;
        }
        const uint32_t pv = Pv & pat, mv = Mv & pat;
        const int d0 = la + __popc(pv & F) - __popc(mv & F), d1 = la + __popc(pv >> 16) - __popc(mv >> 16);
        bool hit0 = valid0 && d0 <= A.limit && e0.rank > rrank;   // a pair is reported from its lower-ranked member
        bool hit1 = valid1 && d1 <= A.limit && e1.rank > rrank;
        if (SUFFIX) {
            hit0 = hit0 && !sk_prefix_within(rmeta >> 8, cfwd0, lb0, A.h, A.k1);
            hit1 = hit1 && !sk_prefix_within(rmeta >> 8, cfwd1, lb1, A.h, A.k1);
        }
        const unsigned long long ball0 = __ballot(hit0), ball1 = __ballot(hit1);
        if (ball0 | ball1) {
            if (hit0) q[nq + __popcll(ball0 & lt)] = (static_cast<unsigned long long>(rrank) << 32) | e0.rank;
            nq += __popcll(ball0);
            if (hit1) q[nq + __popcll(ball1 & lt)] = (static_cast<unsigned long long>(rrank) << 32) | e1.rank;
            nq += __popcll(ball1);
            while (nq >= 64) {
                flush(64);
                for (int k = 64; k < nq; k += 64) {
                    const unsigned long long moved = (k + lane < nq) ? q[k + lane] : 0ull;
                    if (k + lane < nq) q[k - 64 + lane] = moved;
                }
                nq -= 64;
            }
        }
    }
    if (nq) flush(nq);
}

// ---------------------------------------------------------------------------
// device steps (umi_common.hpp); encode_and_rank and pair_edges (umi_host.cpp) run them

static int alloc_umi(const std::string& p, size_t n, UmiArrays* U, int words = 1) {
    U->stride = static_cast<long long>(n);
    SL_TRY(scratch(p + ".code", n * static_cast<size_t>(words), &U->code));
    SL_TRY(scratch(p + ".nmask", n * static_cast<size_t>(words), &U->nmask));
    SL_TRY(scratch(p + ".comp", n, &U->comp));
    SL_TRY(scratch(p + ".meta", n, &U->meta));
    return 0;
}

// Encode at `words` words, in input order: at one word k_umi_encode into "<p>.raw" (strings of more than 32 bases come
// back in too_long / maxlen), beyond k_umi_encode_long into "<p>.rawL" with one sort key per 21 bases of `maxlen`.
int encode_at(const std::string& p, const EncodeIn& in, int words, int maxlen, Encoded* e, hipStream_t s) {
    const int n = in.n;
    int* bad;
    SL_TRY(scratch(p + ".idx", n, &e->idx));
    SL_TRY(scratch(p + ".bad", 3, &bad));
    const int init[3] = {std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), 0};
    SL_HIP(hipMemcpyAsync(bad, init, sizeof init, hipMemcpyHostToDevice, s));
    if (words == 1) {
        SL_TRY(alloc_umi(p + ".raw", n, &e->raw));
        SL_TRY(scratch(p + ".khi", n, &e->khi));
        SL_TRY(scratch(p + ".klo", n, &e->klo));
        hipLaunchKernelGGL(k_umi_encode, dim3(nblk(n, 256)), dim3(256), 0, s, in.chars, in.off, in.members, n, e->raw, e->khi, e->klo, e->idx, in.skip, bad);
    } else {
        const int nkeys = (maxlen + UMI_KEY_BASES - 1) / UMI_KEY_BASES;
        SL_TRY(alloc_umi(p + ".rawL", n, &e->raw, words));
        SL_TRY(scratch(p + ".keysL", static_cast<size_t>(n) * nkeys, &e->keys));
        hipLaunchKernelGGL(k_umi_encode_long, dim3(nblk(n, 256)), dim3(256), 0, s, in.chars, in.off, in.members, n, e->raw, e->keys, e->idx, in.skip, bad, words, nkeys);
    }
    SL_HIP(hipGetLastError());
    int hbad[3];
    SL_HIP(hipMemcpyAsync(hbad, bad, sizeof hbad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    e->bad_char = hbad[0];
    e->too_long = hbad[1];
    e->maxlen = -hbad[2];
    return 0;
}

// Order the encoded set like the trie (most significant: the pre-group) and gather it in that order.
int rank_umis(const std::string& p, const Encoded& e, int words, const int* d_gid, int ngroups, int n, SortedUmis* out, hipStream_t s) {
    unsigned long long *klo = e.klo, *k2;   // one word: the low key of encode_at; beyond: a work buffer for one key plane at a time
    int *idx = e.idx, *idx2;
    SL_TRY(alloc_umi(p + (words > 1 ? ".srtL" : ".srt"), n, &out->U, words));
    if (words > 1) SL_TRY(scratch(p + ".klo", n, &klo));
    SL_TRY(scratch(p + ".k2", n, &k2));
    SL_TRY(scratch(p + ".idx2", n, &idx2));
    if (words > 1) {
        // stable sorts, least-significant key first (only the keys some string reaches)
        const int nkeys = (e.maxlen + UMI_KEY_BASES - 1) / UMI_KEY_BASES;
        int *from = idx, *to = idx2;
        for (int k = nkeys - 1; k >= 0; --k) {
            hipLaunchKernelGGL(k_gather_u64, dim3(nblk(n, 256)), dim3(256), 0, s, e.keys + static_cast<size_t>(k) * n, from, klo, n);
            SL_TRY(radix_sort_pairs(p + ".sorttmp", klo, k2, from, to, n, 63, s));
            std::swap(from, to);
        }
        if (from != idx) SL_HIP(hipMemcpyAsync(idx, from, sizeof(int) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, s));
    } else {
        // least-significant key first; both sorts are stable, ties keep the input order
        SL_TRY(radix_sort_pairs(p + ".sorttmp", klo, k2, idx, idx2, n, 64, s));
        hipLaunchKernelGGL(k_gather_u64, dim3(nblk(n, 256)), dim3(256), 0, s, e.khi, idx2, klo, n);
        SL_TRY(radix_sort_pairs(p + ".sorttmp", klo, k2, idx2, idx, n, 64, s));
    }
    out->gid = nullptr;
    out->ngroups = 1;
    if (d_gid && ngroups > 1) {  // most significant key: the pre-group
        out->ngroups = ngroups;
        int* gsorted;
        SL_TRY(scratch(p + ".gid", n, &gsorted));
        hipLaunchKernelGGL(k_gather_gid, dim3(nblk(n, 256)), dim3(256), 0, s, d_gid, idx, klo, static_cast<int*>(nullptr), n);
        SL_TRY(radix_sort_pairs(p + ".sorttmp", klo, k2, idx, idx2, n, ceil_log2(static_cast<unsigned long long>(ngroups) + 1), s));
        SL_HIP(hipMemcpyAsync(idx, idx2, sizeof(int) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_gather_gid, dim3(nblk(n, 256)), dim3(256), 0, s, d_gid, idx, static_cast<unsigned long long*>(nullptr), gsorted, n);
        out->gid = gsorted;
    }
    hipLaunchKernelGGL(k_gather_umi, dim3(nblk(n, 256)), dim3(256), 0, s, e.raw, idx, out->U, n, words);
    SL_HIP(hipGetLastError());
    out->perm = idx;
    out->n = n;
    out->words = words;
    return 0;
}

// ---- split-key search ----

// hist: strings per length 0..32, [33] strings with an N
int length_hist(const std::string& p, const SortedUmis& S, unsigned int hist[34], hipStream_t s) {
    unsigned int* d_hist;
    SL_TRY(scratch(p + ".sk.hist", 34, &d_hist));
    SL_HIP(hipMemsetAsync(d_hist, 0, 34 * sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_sk_lenhist, dim3(std::min(nblk(S.n, 256), 1024u)), dim3(256), 0, s, S.U, S.n, d_hist);
    SL_HIP(hipMemcpyAsync(hist, d_hist, 34 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

static int sk_prepare(const std::string& p, const SkOrder& O, int h, int k1, bool clip, SkScan* out, hipStream_t s) {
    const int n = O.n;
    int* d_flag; long long* d_pos;
    SL_TRY(scratch(p + ".flag", static_cast<size_t>(n) + 1, &d_flag));
    SL_TRY(scratch(p + ".pos", static_cast<size_t>(n) + 1, &d_pos));
    hipLaunchKernelGGL(k_sk_group_flags, dim3(nblk(n + 1, 256)), dim3(256), 0, s, O, h, d_flag);
    SL_TRY(exclusive_scan(p + ".scantmp", d_flag, d_pos, static_cast<size_t>(n) + 1, s));
    long long nrg = 0;
    SL_HIP(hipMemcpyAsync(&nrg, d_pos + n, sizeof nrg, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    out->O = O;
    out->key = h;
    out->nrg = static_cast<int>(nrg);
    SL_TRY(scratch(p + ".start", static_cast<size_t>(nrg) + 1, &out->rg_start));
    SL_TRY(scratch(p + ".ranges", static_cast<size_t>(nrg) * SK_MAXR + 1, &out->ranges));
    SL_TRY(scratch(p + ".nranges", static_cast<size_t>(nrg) + 1, &out->nranges));
    SL_TRY(scratch(p + ".ctotal", static_cast<size_t>(nrg) + 1, &out->ctotal));
    long long* d_items;
    SL_TRY(scratch(p + ".items", static_cast<size_t>(nrg) + 1, &d_items));
    SL_TRY(scratch(p + ".itemoff", static_cast<size_t>(nrg) + 1, &out->item_off));
    hipLaunchKernelGGL(k_sk_group_starts, dim3(nblk(n + 1, 256)), dim3(256), 0, s, d_flag, d_pos, n, out->rg_start);
    hipLaunchKernelGGL(k_sk_ranges, dim3(nblk(nrg + 1, 64)), dim3(64), 0, s, O, out->rg_start, out->nrg, h, k1, clip ? 1 : 0,
                       out->ranges, out->nranges, out->ctotal, d_items);
    SL_HIP(hipGetLastError());
    SL_TRY(exclusive_scan(p + ".scantmp", d_items, out->item_off, static_cast<size_t>(nrg) + 1, s));
    SL_HIP(hipMemcpyAsync(&out->nitems, out->item_off + nrg, sizeof(long long), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

// Both scan orders with their row groups and candidate ranges.
int split_orders(const std::string& p, const SortedUmis& S, const SkPlan& plan, SplitOrders* out, hipStream_t s) {
    const int n = S.n;
    SkOrder X{}, Y{};
    X.n = Y.n = n;
    X.gid = S.gid;
    SL_TRY(scratch(p + ".sk.elx", static_cast<size_t>(n), &X.el));
    SL_TRY(scratch(p + ".sk.keyx", static_cast<size_t>(n), &X.okey));
    hipLaunchKernelGGL(k_sk_elems<false>, dim3(nblk(n, 256)), dim3(256), 0, s, S.U, n, SK_MIN_LEN, X.el, X.okey, static_cast<int*>(nullptr));
    // reversed strings: sort by key (then by pre-group, stably), carry the trie rank
    SkElem* d_tmp; unsigned long long *d_rk, *d_rk2; int *d_val, *d_val2;
    SL_TRY(scratch(p + ".sk.eltmp", static_cast<size_t>(n), &d_tmp));
    SL_TRY(scratch(p + ".sk.rk", static_cast<size_t>(n), &d_rk));
    SL_TRY(scratch(p + ".sk.rk2", static_cast<size_t>(n), &d_rk2));
    SL_TRY(scratch(p + ".sk.val", static_cast<size_t>(n), &d_val));
    SL_TRY(scratch(p + ".sk.val2", static_cast<size_t>(n), &d_val2));
    SL_TRY(scratch(p + ".sk.ely", static_cast<size_t>(n), &Y.el));
    hipLaunchKernelGGL(k_sk_elems<true>, dim3(nblk(n, 256)), dim3(256), 0, s, S.U, n, SK_MIN_LEN, d_tmp, d_rk, d_val);
    SL_HIP(hipGetLastError());
    SL_TRY(radix_sort_pairs(p + ".sorttmp", d_rk, d_rk2, d_val, d_val2, static_cast<size_t>(n), 63, s));
    Y.okey = d_rk2;
    int* order = d_val2;
    if (S.gid) {
        unsigned long long *d_gk, *d_gk2;
        SL_TRY(scratch(p + ".sk.gk", static_cast<size_t>(n), &d_gk));
        SL_TRY(scratch(p + ".sk.gk2", static_cast<size_t>(n), &d_gk2));
        gid_keys(S.gid, d_val2, n, d_gk, s);
        SL_TRY(radix_sort_pairs(p + ".sorttmp", d_gk, d_gk2, d_val2, d_val, static_cast<size_t>(n), ceil_log2(static_cast<unsigned long long>(S.ngroups) + 1), s));
        order = d_val;
        // keys in the final order
        hipLaunchKernelGGL(k_sk_elems<true>, dim3(nblk(n, 256)), dim3(256), 0, s, S.U, n, SK_MIN_LEN, d_tmp, d_rk, d_val2);
        hipLaunchKernelGGL(k_gather_u64, dim3(nblk(n, 256)), dim3(256), 0, s, d_rk, order, d_rk2, n);
        SL_TRY(scratch(p + ".sk.gidy", static_cast<size_t>(n), &Y.gid));
    }
    hipLaunchKernelGGL(k_sk_permute, dim3(nblk(n, 256)), dim3(256), 0, s, d_tmp, order, S.gid, n, Y.el, Y.gid);
    SL_HIP(hipGetLastError());
    // row groups and ranges once per key length in use; the prefix scan starts at the row group itself (columns
    // ranked below the row report the pair themselves)
    const bool clip = true;
    out->fwd.clear(); out->rev.clear();
    for (const SkClass& c : plan.classes) {
        bool have = false;
        for (const SkScan& q : out->fwd) have = have || q.key == c.h;
        if (!have) { out->fwd.emplace_back(); SL_TRY(sk_prepare(p + ".skx" + std::to_string(c.h), X, c.h, plan.k1, clip, &out->fwd.back(), s)); }
        have = false;
        for (const SkScan& q : out->rev) have = have || q.key == c.s;
        if (!have) { out->rev.emplace_back(); SL_TRY(sk_prepare(p + ".sky" + std::to_string(c.s), Y, c.s, plan.k2, false, &out->rev.back(), s)); }
    }
    return 0;
}

// The scans of the plan's classes, prefix then suffix; *items: work items of the launches, *two_columns: launches of k_sk_scan_pk.
void split_scans(const SplitOrders& O, const SearchPlan& P, unsigned stride, const PairBuffer& b, long long* items, int* two_columns, hipStream_t s) {
    *items = 0;
    *two_columns = 0;
    for (const SkClass& c : P.sk.classes)
        for (int pass = 0; pass < 2; ++pass) {
            const SkScan* Q = nullptr;
            for (const SkScan& q : pass ? O.rev : O.fwd) if (q.key == (pass ? c.s : c.h)) Q = &q;
            if (!Q) continue;
            const long long blocks = (Q->nitems + stride - 1) / stride;
            if (blocks <= 0) continue;
            *items += Q->nitems;
            *two_columns += c.two ? 1 : 0;
            const SkScanArgs a{Q->O.el, Q->rg_start, Q->nrg, Q->ranges, Q->nranges, Q->ctotal, Q->item_off, stride, P.limit, c.h, P.sk.k1,
                               c.len_lo, c.len_hi, P.row_lo, P.row_hi, b.edges, b.count, b.cap};
            pick([&](auto two_, auto suffix_) {
                constexpr bool SUFFIX = decltype(suffix_)::value != 0;
                if constexpr (decltype(two_)::value != 0) hipLaunchKernelGGL(k_sk_scan_pk<SUFFIX>, dim3(static_cast<unsigned>(blocks)), dim3(SK_COLS / 2), 0, s, a);
                else hipLaunchKernelGGL(k_sk_scan<SUFFIX>, dim3(static_cast<unsigned>(blocks)), dim3(SK_COLS), 0, s, a);
                return 0;
            }, Ints<0, 1>{}, c.two, Ints<0, 1>{}, pass);
        }
}

// ---- tile search ----

// Tile pairs that can hold neighbours (see k_tile_pairs), and the prefixes of the 64-element blocks for the sub-tile
// filter inside the pair kernel.
int tile_filter(const std::string& p, const SortedUmis& S, const SearchPlan& P, TileList* out, hipStream_t s) {
    const int n = S.n, nt = P.nt;
    TileInfo* d_info; uint32_t* d_l; unsigned int* d_lc;
    SL_TRY(scratch(p + ".tinfo", static_cast<size_t>(nt), &d_info));
    // the list is bounded by the upper triangle of the launch
    const size_t max_list = static_cast<size_t>(P.tile_hi - P.tile_lo) * static_cast<size_t>(nt);
    SL_TRY(scratch(p + ".tlist", max_list, &d_l));
    SL_TRY(scratch(p + ".tcount", 1, &d_lc));
    SL_HIP(hipMemsetAsync(d_lc, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_tile_info<TILE>, dim3(static_cast<unsigned>(nt)), dim3(TILE), 0, s, S.U, S.gid, n, std::max(P.special_lreq, 0), d_info);
    TileInfo* d_sub;
    const unsigned nsub = nblk(n, 64);
    SL_TRY(scratch(p + ".tsub", static_cast<size_t>(nsub), &d_sub));
    hipLaunchKernelGGL(k_tile_info<64>, dim3(nsub), dim3(64), 0, s, S.U, S.gid, n, 0, d_sub);
    const int rc = pick([&](auto l_) {
        hipLaunchKernelGGL(k_tile_pairs<decltype(l_)::value>, dim3(nblk(nt, 256), static_cast<unsigned>(P.tile_hi - P.tile_lo)), dim3(256), 0, s,
                           d_info, nt, P.tile_lo, P.tile_hi, P.split ? 1 : 0, d_l, d_lc);
        return 0;
    }, Ints<0, 1, 2, 3, 4, 5>{}, P.L);
    if (rc == NO_KERNEL) return fail("sarlacc_amd: internal error: no tile filter for prefix distance %d", P.L);
    SL_HIP(hipGetLastError());
    SL_HIP(hipMemcpyAsync(&out->n, d_lc, sizeof out->n, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    out->list = d_l;
    out->sub = d_sub;
    return 0;
}

// The plan's tile-pair kernel: over the listed tile pairs (every stride-th of them: a sample), or over every pair of a
// row tile of the plan with a tile of the set.
int pair_search(const SortedUmis& S, const SearchPlan& P, const TileList& T, unsigned stride, const PairBuffer& b, hipStream_t s) {
    if (P.tile_hi <= P.tile_lo) return 0;
    const PairArgs a{S.U, S.gid, S.n, 2 * P.limit, b.edges, b.count, b.cap, P.tile_lo, T.list, T.sub, stride, P.special_lreq};
    const dim3 grid = T.list ? dim3(T.n / stride) : dim3(static_cast<unsigned>(P.tile_hi - P.tile_lo), static_cast<unsigned>(P.nt));
    if (grid.x == 0) return 0;
    int rc;
    if (P.words > 1)
        rc = pick([&](auto k_, auto xl_) {
            hipLaunchKernelGGL((k_umi_pairs_long<decltype(k_)::value, decltype(xl_)::value != 0>), grid, dim3(TILE), 0, s, a);
            return 0;
        }, Ints<0, 1, 2, 3, 5, 8, 16, PAIRS_K_FULL>{}, P.K, Ints<0, 1>{}, P.xl);
    else
        rc = pick([&](auto k_) {
            hipLaunchKernelGGL(k_umi_pairs<decltype(k_)::value>, grid, dim3(TILE), 0, s, a);
            return 0;
        }, Ints<0, 1, 2, 3, 4, 5, 8, 16, UMI_MAXLEN>{}, P.K);
    return rc != NO_KERNEL ? rc : fail("sarlacc_amd: internal error: no tile-pair kernel for band %d at %d words", P.K, P.words);
}

}  // namespace sarlacc
