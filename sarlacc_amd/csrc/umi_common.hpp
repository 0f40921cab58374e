// umi_common.hpp -- what the UMI sources share: string constants and layout, workspace names, the doubled masked
// Levenshtein distance on one-word and multi-word operands, the plan structs and the device steps.  The stage is split
// like the align, MSA and consensus stages:
//   umi_host.cpp     everything that decides: the C entry points, the search plan and the sample / retry loop
//                    (pair_edges), the words decision of the encode, the clustering's round control (cluster_dev), every
//                    user-facing error, counter and timer
//   umi_search.hip   kernels and device steps of the encoding, the tile search and the split-key search
//   umi_cluster.hip  kernels and device steps of the greedy clustering
//   umi.hip          kernels and device steps of the adjacency, the dense distances and the pair check
// A kernel is launched only from the file that defines it; the .hip files hold no policy (see "device steps" below).
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
// sarlacc_release_umi_workspace (umi_host.cpp) gives back exactly the UMI stage's buffers.
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
// what travels between the steps

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

// ---------------------------------------------------------------------------
// the search plan (made by pair_edges, umi_host.cpp; turned into launches by pair_search and split_scans)

constexpr int SK_MIN_LEN = 8;            // shorter strings are "special" (keys under 4 bases select too much)
constexpr int SK_MAX_KEY = 8;            // bases per key at most (9 bases of the forward string travel with every element)

struct SkClass { int len_lo, len_hi, h, s; bool two; };   // rows of lengths len_lo..len_hi scan with keys of h and s bases; two: by k_sk_scan_pk

struct SkPlan {
    std::vector<SkClass> classes;   // row lengths present in the set, with the key lengths they scan with
    int k1 = 0, k2 = 0;             // edits allowed in the prefix / suffix key
    long long nspecial = 0;
};

constexpr int PAIRS_K_FULL = -1;    // SearchPlan::K: the long kernels' full DP
constexpr int PAIRS_K_NONE = -2;    // SearchPlan::K: no tile-pair kernel in the plan

struct SearchPlan {
    int limit = 0;
    int words = 1;                  // SortedUmis::words
    bool xl = false;                // more than UMI_LONG_WORDS words: k_umi_pairs_long<K, true>
    int K = PAIRS_K_NONE;           // template K of k_umi_pairs / k_umi_pairs_long
    bool split = false;             // the split-key scans run, by `sk`
    SkPlan sk;
    bool tiles = true;              // the tile-pair kernel is part of the search (split: for the pairs with a special member)
    bool filter = false;            // k_tile_info and k_tile_pairs<L> list the tile pairs to search
    int L = 0;
    int special_lreq = -1;          // PairArgs::special_lreq
    int nt = 0, tile_lo = 0, tile_hi = 0;   // tiles of the set; the row tiles of this search
    uint32_t row_lo = 0, row_hi = 0;        // the same as trie ranks
    bool sample_tiles = false;      // a sampled pass may run first: over every sample_stride-th listed tile pair ...
    bool sample_items = false;      // ... and work item of the scans; it runs when either has SAMPLE_MIN entries
};

struct SkElem;
struct TileInfo;

struct SkOrder {
    SkElem* el;                  // [n] in scan order
    unsigned long long* okey;    // [n] 3 bits per base (A..T = 1..4, N = 5, past the end = 0), first 21 bases, in scan order
    int* gid;                    // [n] pre-group in scan order (nullptr: one group)
    int n;
};

struct SkScan {          // one scan order with row groups for one key length, ready to launch
    SkOrder O{};
    int key = 0;
    int* rg_start = nullptr;
    int nrg = 0;
    int2* ranges = nullptr;
    int *nranges = nullptr, *ctotal = nullptr;
    long long* item_off = nullptr;
    long long nitems = 0;
};

struct SplitOrders { std::vector<SkScan> fwd, rev; };

struct TileList {               // what the tile filter kept (list == nullptr: no filter, every tile pair is searched)
    const uint32_t* list = nullptr;
    const TileInfo* sub = nullptr;
    unsigned int n = 0;
};

struct PairBuffer { unsigned long long *edges, *count, cap; };

// ---------------------------------------------------------------------------
// clustering state (umi_cluster.hip's kernels take it by value; cluster_dev, umi_host.cpp, runs the rounds)

struct ClusterState {
    const long long* off;
    const int* nbr;
    int n;
    int* remaining;
    int* state;                 // 0 live, 1 solo, 2 clustered
    int* mark;                  // round in which the node was clustered
    unsigned long long* key;
    unsigned long long* m1;
    int* seed;                  // 1 if picked as a seed (any round)
    unsigned long long* pickkey;
    int* memb;                  // members of the cluster seeded at v, stored at off[v]..
    int* csize;
    int* err;                   // [0] min index with empty list, [1] min index bad solo, [2] missing self / asymmetric, [3] a node twice
    int* live;                  // count of live pool nodes this round
};

struct ClusterTop {             // candidate-set rounds, see umi_cluster.hip
    int* maxrem;                // largest remaining of a live node, this round
    int* cand;                  // candidate list
    int* counts;                // [0] candidates, [1] picks, [2] 1 when the list was cut off at `cap`, [3] nodes clustered this round
    unsigned long long* hop1;
    int cap;
    int* marked;                // the nodes clustered this round (two picks of a round share no neighbour: no node twice)
    int* ctl;                   // the rounds' control block, see k_cl_control
};
// (the host's write-back after a full round covers CTL_MODE..CTL_WAS_TOP only: the counts behind them survive it)
enum { CTL_MODE, CTL_DELTA, CTL_WAS_TOP, CTL_ROUNDS, CTL_MAXREM, CTL_WIDENED, CTL_NARROWED, CTL_N = 8 };
enum { CL_DONE = 0, CL_TOP = 1, CL_WANTS_FULL = 3 };   // CL_WANTS_FULL: the list was cut off -- the host runs one round over every list
constexpr int CL_GROUP = 8;     // candidate-set rounds per read-back of the control block

// ---------------------------------------------------------------------------
// device steps: device arrays and sizes in, kernels / scans / sorts enqueued on the stream, device arrays out.  A step may
// name scratch and read back the one size its own output needs; it decides nothing, sets no counter and raises only HIP
// and allocation errors (and, in tile_filter and pair_search, an "internal error" when the plan names a template instance
// the library is not built with: unreachable while plan_search and their Ints<...> lists agree).

struct EncodeIn {
    const uint8_t* chars; const int64_t* off;
    const int32_t* members;     // optional 1-based ids selecting the strings
    const uint8_t* skip;        // optional: elements encoded as empty strings
    int n;
};
struct Encoded {
    UmiArrays raw;              // in input order: "<p>.raw" at one word, "<p>.rawL" beyond
    unsigned long long *khi, *klo, *keys;   // sort keys: two at one word, (maxlen + 20) / 21 planes beyond
    int* idx;
    int bad_char, too_long;     // first string with a character outside ACGTN / of more than 32 bases (INT_MAX: none)
    int maxlen;                 // of the strings of more than 32 bases
};

// umi_search.hip
int encode_at(const std::string& p, const EncodeIn& in, int words, int maxlen, Encoded* e, hipStream_t s);
int rank_umis(const std::string& p, const Encoded& e, int words, const int* d_gid, int ngroups, int n, SortedUmis* out, hipStream_t s);
int length_hist(const std::string& p, const SortedUmis& S, unsigned int hist[34], hipStream_t s);
int split_orders(const std::string& p, const SortedUmis& S, const SkPlan& plan, SplitOrders* out, hipStream_t s);
int tile_filter(const std::string& p, const SortedUmis& S, const SearchPlan& P, TileList* out, hipStream_t s);
void split_scans(const SplitOrders& O, const SearchPlan& P, unsigned stride, const PairBuffer& b, long long* items, int* two_columns, hipStream_t s);
int pair_search(const SortedUmis& S, const SearchPlan& P, const TileList& T, unsigned stride, const PairBuffer& b, hipStream_t s);

// umi.hip
struct SelfLinks { int* flag; long long* pos; long long n; };
int self_links(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single, SelfLinks* out, hipStream_t s);
int directed_keys(const std::string& p, const SortedUmis& S, const unsigned long long* d_edges, unsigned long long m,
                  const SelfLinks& self, DirectedKeys* out, hipStream_t s);
int adjacency_from_keys(const unsigned long long* keys, long long nk, const int* perm, int n, DevAdj* adj, hipStream_t s);
int link_set(const std::string& p, const DirectedKeys& K, const int* perm, unsigned long long** d_set, hipStream_t s);
int links_in_set(const std::string& p, const DirectedKeys& K, const int* perm, const unsigned long long* d_set, long long nset,
                 DirectedKeys* kept, hipStream_t s);
int check_pairs(const unsigned long long* d_edges, long long npairs, long long n, int* bad, hipStream_t s);
int dense_distances(const std::string& p, const UmiArrays& U, int n, int words, double** d_out, hipStream_t s);

// umi_cluster.hip
void gid_keys(const int* gid, const int* val, long long n, unsigned long long* key, hipStream_t s);
int cluster_begin(const DevAdj& adj, int n, bool check_sym, ClusterState* S, int herr[4], hipStream_t s);
int cluster_candidates_begin(const ClusterState& S, bool control, ClusterTop* T, hipStream_t s);
int cluster_count_live(const ClusterState& S, int* live, hipStream_t s);
void rounds_candidates(const ClusterState& S, const ClusterTop& T, int* round, hipStream_t s);
void round_dense(const ClusterState& S, int round, hipStream_t s);
void round_sparse(const ClusterState& S, int round, hipStream_t s);
int clusters_write(const ClusterState& S, const int32_t* d_members, const int* d_gid, int ngroups, ClusterResult* res, hipStream_t s);

}  // namespace sarlacc
