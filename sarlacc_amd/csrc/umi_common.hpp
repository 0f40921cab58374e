// umi_common.hpp -- what the UMI sources share: string constants and layout, workspace names, the doubled masked
// Levenshtein distance on one-word and multi-word operands, and the host interfaces between
//   umi_search.hip   encoding, tile search, split-key search (pair_edges, neighbour_keys)
//   umi_cluster.hip  greedy clustering (cluster_dev)
//   umi.hip          adjacency, dense distances, the entry points and the pair exchange
#pragma once

#include "common.hpp"
#include "devprim.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace sarlacc {

constexpr int UMI_MAXLEN = 32;        // one 64-bit word of 2-bit codes: the fast path (all filters, queued DP)
constexpr int UMI_LONG_WORDS = 4;     // strings of 33..128 bases: the same search on 4-word codes (k_umi_pairs_long)
constexpr int UMI_LONG_MAX = 32 * UMI_LONG_WORDS;
constexpr int UMI_XL_WORDS = 32;      // strings of 129..1024 bases: as many words as the longest string needs, read from HBM (k_umi_pairs_long<K, true>)
constexpr int UMI_XL_MAX = 32 * UMI_XL_WORDS;
// meta word of a string: length | number of N << 12 (12 bits each)
__host__ __device__ __forceinline__ int umi_len(uint32_t meta) { return static_cast<int>(meta & 0xfffu); }
__host__ __device__ __forceinline__ int umi_nn(uint32_t meta) { return static_cast<int>((meta >> 12) & 0xfffu); }
constexpr uint32_t UMI_META_NONE = 0xffffffu;   // a padding column: length 4095, never within any limit of a real string
constexpr int UMI_KEY_BASES = 21;     // bases per 64-bit sort key (3 bits each)
constexpr int TILE = 256;
constexpr int INF_D = 1 << 20;

// Workspace names.  Every device buffer of the UMI code is named "<prefix>.<what>" with a prefix of this table, so that
// sarlacc_release_umi_workspace (umi.hip) gives back exactly the UMI stage's buffers.
enum UmiWs { WS_U1, WS_U2, WS_G1, WS_G2, WS_G, WS_PS, WS_LV, WS_LEV, WS_ADJ, WS_CL, WS_N };
inline constexpr const char* UMI_WS[WS_N] = {
    "u1", "u2",           // encode_and_rank and the searches of UMI1 / UMI2
    "g1", "g2", "g",      // sarlacc_umi_group: the strings, the pre-group tables
    "ps", "lv", "lev",    // the strings of the pair exchange, fast_levdist_test, compute_lev_masked
    "adj", "cl"};         // neighbour lists, clustering

struct UmiArrays {
    unsigned long long* code;   // 2 bits per base (N stored as 0); word w of string s at code[w * stride + s]
    uint32_t* nmask;            // bit i set: base i is N; same layout
    uint32_t* comp;             // counts of A,C,G,T, one byte each
    uint32_t* meta;             // len | nN << 12 (umi_len, umi_nn)
    long long stride;           // strings per word plane (one plane on the fast path)
};

// ---------------------------------------------------------------------------
// distance operands: base i (0-based) and whether it is N

// a string of up to 32 bases, code and N mask in registers
struct WordStr {
    static constexpr bool in_registers = true;
    unsigned long long code;
    uint32_t nmask;
    __device__ __forceinline__ unsigned base(int i) const { return static_cast<unsigned>(code >> (2 * i)) & 3u; }
    __device__ __forceinline__ unsigned isn(int i) const { return (nmask >> i) & 1u; }
};

// a multi-word string whose word planes lie `plane` elements apart
struct LongStr {
    static constexpr bool in_registers = false;
    const unsigned long long* code;
    const uint32_t* nmask;
    int plane;
    __device__ __forceinline__ unsigned base(int i) const { return static_cast<unsigned>(code[(i >> 5) * plane] >> (2 * (i & 31))) & 3u; }
    __device__ __forceinline__ unsigned isn(int i) const { return (nmask[(i >> 5) * plane] >> (i & 31)) & 1u; }
};

// Doubled masked Levenshtein distance restricted to the band |i-j| <= K, the band in registers; returns
// INF_D as soon as every cell of a row exceeds lim2 (src/sorted_trie.cpp:13-21 costs).  A one-word operand is read in
// place: through base() / isn() the compiler turns every cell's branch into selects, and k_lev_dense then spills.
template <int K, typename Str>
__device__ __forceinline__ int banded_lev2(const Str a, int la, const Str b, int lb, int lim2) {
    constexpr int BW = 2 * K + 1;
    int v[BW];
#pragma unroll
    for (int d = 0; d < BW; ++d) {
        const int i = d - K;
        v[d] = (i >= 0 && i <= la) ? 2 * i : INF_D;
    }
    for (int j = 1; j <= lb; ++j) {
        unsigned cbj, nbj;
        if constexpr (Str::in_registers) {
            cbj = static_cast<unsigned>(b.code >> (2 * (j - 1))) & 3u;
            nbj = (b.nmask >> (j - 1)) & 1u;
        } else {
            cbj = b.base(j - 1);
            nbj = b.isn(j - 1);
        }
        int rowmin = INF_D, left = INF_D;
#pragma unroll
        for (int d = 0; d < BW; ++d) {
            const int i = j + d - K;
            int best = INF_D;
            if (i >= 0 && i <= la) {
                if (i == 0) {
                    best = 2 * j;
                } else {
                    int sub;
                    if constexpr (Str::in_registers) {
                        const unsigned nai = (a.nmask >> (i - 1)) & 1u;
                        const unsigned cai = static_cast<unsigned>(a.code >> (2 * (i - 1))) & 3u;
                        sub = (nai | nbj) ? 1 : (cai == cbj ? 0 : 2);
                    } else {
                        sub = (a.isn(i - 1) | nbj) ? 1 : (a.base(i - 1) == cbj ? 0 : 2);
                    }
                    best = v[d] + sub;
                    if (d + 1 < BW) best = min(best, v[d + 1] + 2);
                    best = min(best, left + 2);
                }
            }
            v[d] = best;
            left = best;
            rowmin = min(rowmin, best);
        }
        if (rowmin > lim2) return INF_D;
    }
    const int dd = la - lb + K;
    int res = INF_D;
#pragma unroll
    for (int d = 0; d < BW; ++d) res = (d == dd) ? v[d] : res;
    return res;
}

// full (unbanded) doubled masked Levenshtein distance, one row in thread-private memory; gives up with
// INF_D once a whole row exceeds lim2.  For thresholds beyond 16 and for the dense distances.
template <int MAXL, typename Str>
__device__ __forceinline__ int full_lev2(const Str a, int la, const Str b, int lb, int lim2) {
    int row[MAXL + 1];
    for (int i = 0; i <= la; ++i) row[i] = 2 * i;
    for (int j = 1; j <= lb; ++j) {
        const unsigned cbj = b.base(j - 1), nbj = b.isn(j - 1);
        int diag = row[0];
        row[0] = 2 * j;
        int rowmin = row[0];
        for (int i = 1; i <= la; ++i) {
            const int sub = (a.isn(i - 1) | nbj) ? 1 : (a.base(i - 1) == cbj ? 0 : 2);
            const int best = min(diag + sub, min(row[i] + 2, row[i - 1] + 2));
            diag = row[i];
            row[i] = best;
            rowmin = min(rowmin, best);
        }
        if (rowmin > lim2) return INF_D;
    }
    return row[la];
}

// ---------------------------------------------------------------------------
// host interfaces between the UMI sources

struct SortedUmis {
    UmiArrays U;   // in (pre-group, trie) order
    int* perm;     // rank -> local index
    int* gid;      // pre-group per rank (nullptr: a single group)
    int n;
    int words;     // 1: every string has at most 32 bases; UMI_LONG_WORDS up to 128 bases; beyond, what the longest string needs
    int ngroups;   // pre-groups (1 when gid is nullptr)
    int nskip = 0;       // elements that are never compared (pre-groups of one read: encoded as empty strings)
    int max_group = 0;   // size of the largest pre-group (0: unknown, the whole set)
};

struct DirectedKeys {
    unsigned long long* keys;  // sorted (orig_row << 32 | column rank)
    long long nk;
};

struct DevAdj {
    long long* off;  // [n+1]
    int* nbr;        // local 0-based ids, trie order
    long long nnz;
};

struct ClusterResult {
    long long nclu = 0;
    long long* d_coff = nullptr;  // [nclu+1]
    int32_t* d_out = nullptr;     // member ids (1-based; mapped through members when given)
    long long total = 0;
};

// umi_search.hip
__global__ void k_umi_encode(const uint8_t* chars, const int64_t* off, const int32_t* members, int n, UmiArrays U,
                             unsigned long long* key_hi, unsigned long long* key_lo, int* idx, const uint8_t* skip, int* bad);
__global__ void k_umi_encode_long(const uint8_t* chars, const int64_t* off, const int32_t* members, int n, UmiArrays U,
                                  unsigned long long* keys, int* idx, const uint8_t* skip, int* bad, int words, int nkeys);
int alloc_umi(const std::string& p, size_t n, UmiArrays* U, int words = 1);
int encode_and_rank(const std::string& p, const uint8_t* d_chars, const int64_t* d_off, const int32_t* d_members,
                    const int* d_gid, int ngroups, int n, SortedUmis* out, hipStream_t s, const uint8_t* d_skip = nullptr,
                    int nskip = 0, int max_group = 0);
int pair_edges(const std::string& p, const SortedUmis& S, int limit, int tile_lo, int tile_hi,
               unsigned long long** d_edges_out, unsigned long long* m_out, hipStream_t s);
int neighbour_keys(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single, DirectedKeys* out, hipStream_t s);

// umi.hip
int keys_from_edges(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single,
                    const unsigned long long* d_edges, unsigned long long m, DirectedKeys* out, hipStream_t s);

// umi_cluster.hip
__global__ void k_cl_gidkey(const int* gid, const int* val, long long n, unsigned long long* key);
int cluster_dev(const DevAdj& adj, int n, const int32_t* d_members, const int* d_gid, int ngroups, bool check_sym,
                ClusterResult* res, hipStream_t s);

}  // namespace sarlacc
