// umi.hip -- the UMI stage's adjacency, dense distances and entry points on gfx950.
// Replaces compute_lev_masked (the reference's src/compute_lev_masked.cpp:13-64) and the per pre-group driver umi_group
// (src/umi_group.cpp:14-116).  Directed adjacency is a radix sort of (row << 32 | column-rank) keys of the undirected
// pairs of the search (umi_search.hip); the greedy clustering is in umi_cluster.hip.  Design: DESIGN.md "UMI stage".
#include "umi_common.hpp"

#include "../../include/sarlacc_amd.h"

namespace sarlacc {

// ---------------------------------------------------------------------------
// dense distances for compute_lev_masked: out in R 'dist' order (i-major lower triangle), value = d2 / 2 (multiples
// of 0.5 are exact in fp64); dense_pair inverts the pair index p -> (i, j), i < j, i-major
__device__ __forceinline__ void dense_pair(long long p, int n, long long& i, long long& j) {
    i = static_cast<long long>((2.0 * n - 1 - sqrt((2.0 * n - 1) * (2.0 * n - 1) - 8.0 * p)) / 2);
    auto start = [&](long long r) { return r * (2LL * n - r - 1) / 2; };
    while (i > 0 && start(i) > p) --i;
    while (start(i + 1) <= p) ++i;
    j = i + 1 + (p - start(i));
}

template <int MAXL>
__global__ void k_lev_dense_long(UmiArrays U, int n, double* out) {
    const long long p = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    const long long npairs = static_cast<long long>(n) * (n - 1) / 2;
    if (p >= npairs) return;
    long long i, j;
    dense_pair(p, n, i, j);
    const LongStr a{U.code + i, U.nmask + i, static_cast<int>(U.stride)}, b{U.code + j, U.nmask + j, static_cast<int>(U.stride)};
    const int d = full_lev2<MAXL>(a, umi_len(U.meta[i]), b, umi_len(U.meta[j]), 8 * MAXL);
    out[p] = static_cast<double>(d) / 2.0;
}

__global__ void k_lev_dense(UmiArrays U, int n, double* out) {
    const long long p = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    const long long npairs = static_cast<long long>(n) * (n - 1) / 2;
    if (p >= npairs) return;
    long long i, j;
    dense_pair(p, n, i, j);
    const uint32_t ma = U.meta[i], mb = U.meta[j];
    const int d = banded_lev2<UMI_MAXLEN>(WordStr{U.code[i], U.nmask[i]}, umi_len(ma), WordStr{U.code[j], U.nmask[j]}, umi_len(mb), 4 * UMI_MAXLEN);
    out[p] = static_cast<double>(d) / 2.0;
}

// ---------------------------------------------------------------------------
// adjacency

// undirected rank pairs -> directed keys (orig_row << 32 | column rank), plus self links
__global__ void k_expand_edges(const unsigned long long* edges, unsigned long long m, const int* perm,
                               unsigned long long* keys) {
    const unsigned long long e = blockIdx.x * static_cast<unsigned long long>(blockDim.x) + threadIdx.x;
    if (e >= m) return;
    const unsigned ri = static_cast<unsigned>(edges[e] >> 32), rj = static_cast<unsigned>(edges[e]);
    keys[2 * e] = (static_cast<unsigned long long>(perm[ri]) << 32) | rj;
    keys[2 * e + 1] = (static_cast<unsigned long long>(perm[rj]) << 32) | ri;
}

// single: pre-groups of one read pass through untouched (src/umi_group.cpp:39-42): they always
// get their self link so that the clustering emits them as solos without any check
__global__ void k_self_flags(UmiArrays U, int n, int lim2, const uint8_t* single, const int* perm, int* flag) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const bool self = umi_nn(U.meta[r]) <= lim2;  // d2(x,x) = #N (App.B Q10)
    flag[r] = (self || (single && single[perm[r]])) ? 1 : 0;
}

__global__ void k_self_keys(const int* flag, const long long* pos, const int* perm, int n, unsigned long long* keys) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && flag[r]) keys[pos[r]] = (static_cast<unsigned long long>(perm[r]) << 32) | static_cast<unsigned>(r);
}

// sorted keys (row << 32 | x) -> row offsets
__global__ void k_row_offsets(const unsigned long long* keys, long long nk, int n, long long* off) {
    const long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (i > nk) return;
    const long long prev = (i == 0) ? -1 : static_cast<long long>(keys[i - 1] >> 32);
    const long long cur = (i == nk) ? n : static_cast<long long>(keys[i] >> 32);
    for (long long r = prev + 1; r <= cur; ++r) off[r] = i;
}

__global__ void k_cols_from_keys(const unsigned long long* keys, long long nk, const int* perm, int* nbr) {
    const long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (i < nk) nbr[i] = perm[static_cast<unsigned>(keys[i])];
}

// (row << 32 | rank) -> (row << 32 | orig col)
__global__ void k_keys_to_orig(const unsigned long long* keys, long long nk, const int* perm, unsigned long long* out) {
    const long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (i < nk) out[i] = (keys[i] & 0xffffffff00000000ull) | static_cast<unsigned>(perm[static_cast<unsigned>(keys[i])]);
}

// keep[i] = 1 if (row, perm2[rank]) of keys2[i] is present in the sorted set s1
__global__ void k_intersect_flags(const unsigned long long* keys2, long long nk2, const int* perm2,
                                  const unsigned long long* s1, long long n1, int* keep) {
    const long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (i >= nk2) return;
    const unsigned long long want = (keys2[i] & 0xffffffff00000000ull) | static_cast<unsigned>(perm2[static_cast<unsigned>(keys2[i])]);
    long long lo = 0, hi = n1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (s1[mid] < want) lo = mid + 1; else hi = mid;
    }
    keep[i] = (lo < n1 && s1[lo] == want) ? 1 : 0;
}

__global__ void k_compact_keys(const unsigned long long* keys, const int* keep, const long long* pos, long long nk,
                               unsigned long long* out) {
    const long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (i < nk && keep[i]) out[pos[i]] = keys[i];
}

// ---------------------------------------------------------------------------
// host orchestration

// number of pairs the last sarlacc_dev_umi_pairs_shard of this thread left in the workspace buffer "u1.edges" (-1: none);
// every pair_edges call on "u1" reuses that buffer, so it is reset before one
static thread_local long long g_shard_pairs = -1;

// Directed, sorted adjacency keys (self links included) from undirected rank pairs.
int keys_from_edges(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single,
                    const unsigned long long* d_edges, unsigned long long m, DirectedKeys* out, hipStream_t s) {
    const int n = S.n;
    const int lim2 = 2 * limit;
    int* d_flag; long long* d_pos;
    SL_TRY(scratch(p + ".sflag", static_cast<size_t>(n) + 1, &d_flag));
    SL_TRY(scratch(p + ".spos", static_cast<size_t>(n) + 1, &d_pos));
    hipLaunchKernelGGL(k_self_flags, dim3(nblk(n, 256)), dim3(256), 0, s, S.U, n, lim2, d_single, S.perm, d_flag);
    SL_HIP(hipMemsetAsync(d_flag + n, 0, sizeof(int), s));
    SL_TRY(exclusive_scan(p + ".scantmp", d_flag, d_pos, static_cast<size_t>(n) + 1, s));
    long long nself = 0;
    SL_HIP(hipMemcpyAsync(&nself, d_pos + n, sizeof nself, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    const long long nk = 2 * static_cast<long long>(m) + nself;
    // The neighbour lists are explicit (as the reference's are, src/umi_group.cpp:59-103): 20 bytes per link while they are
    // sorted.  Measured up to 2.8e9 links (7e5 12-base UMIs at threshold 4: 4 000 neighbours each); beyond 2^32 the
    // call stops here instead of running out of memory half way.
    if (nk > 0xFFFFFFFFll)
        return fail("sarlacc_amd: %lld neighbour links in one call (at most 4294967295): the threshold joins most of the set -- "
                    "lower it or split the reads into pre-groups", nk);
    unsigned long long *d_k0, *d_k1;
    SL_TRY(scratch(p + ".k0", static_cast<size_t>(nk), &d_k0));
    SL_TRY(scratch(p + ".k1", static_cast<size_t>(nk), &d_k1));
    if (m) hipLaunchKernelGGL(k_expand_edges, dim3(nblk(static_cast<long long>(m), 256)), dim3(256), 0, s, d_edges, m, S.perm, d_k0 + nself);
    hipLaunchKernelGGL(k_self_keys, dim3(nblk(n, 256)), dim3(256), 0, s, d_flag, d_pos, S.perm, n, d_k0);
    SL_HIP(hipGetLastError());
    if (nk) SL_TRY(radix_sort_keys(p + ".sorttmp", d_k0, d_k1, static_cast<size_t>(nk), 32 + ceil_log2(static_cast<unsigned long long>(n) + 1), s));
    out->keys = d_k1;
    out->nk = nk;
    return 0;
}

static int adjacency_from_keys(const unsigned long long* keys, long long nk, const int* perm, int n, DevAdj* adj, hipStream_t s) {
    const std::string p = UMI_WS[WS_ADJ];
    SL_TRY(scratch(p + ".off", static_cast<size_t>(n) + 1, &adj->off));
    SL_TRY(scratch(p + ".nbr", static_cast<size_t>(nk), &adj->nbr));
    hipLaunchKernelGGL(k_row_offsets, dim3(nblk(nk + 1, 256)), dim3(256), 0, s, keys, nk, n, adj->off);
    if (nk) hipLaunchKernelGGL(k_cols_from_keys, dim3(nblk(nk, 256)), dim3(256), 0, s, keys, nk, perm, adj->nbr);
    SL_HIP(hipGetLastError());
    adj->nnz = nk;
    return 0;
}

// Neighbour lists for one group: UMI1 only, or UMI1 n UMI2 listed in UMI2's order
// (src/umi_group.cpp:59-103).
static int group_adjacency(const uint8_t* d_c1, const int64_t* d_o1, const uint8_t* d_c2, const int64_t* d_o2,
                           const int32_t* d_members, const int* d_gid, const uint8_t* d_single, int ngroups, int n,
                           int limit1, int limit2, DevAdj* adj, hipStream_t s, int nsingle = 0, int max_group = 0) {
    const std::string u1 = UMI_WS[WS_U1], u2 = UMI_WS[WS_U2];
    SortedUmis S1;
    DirectedKeys K1;
    auto now = [&] { (void)hipStreamSynchronize(s); return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    SL_TRY(encode_and_rank(u1, d_c1, d_o1, d_members, d_gid, ngroups, n, &S1, s, d_single, nsingle, max_group));
    const double t1 = now();
    g_shard_pairs = -1;
    SL_TRY(neighbour_keys(u1, S1, limit1, d_single, &K1, s));
    const double t2 = now();
    ctx().counts["umi_encode_sort_s"] = t1 - t0;
    ctx().counts["umi_search_and_key_sort_s"] = t2 - t1;
    if (!d_c2) return adjacency_from_keys(K1.keys, K1.nk, S1.perm, n, adj, s);

    // membership set of UMI1 links keyed by original column id
    unsigned long long *d_s1a, *d_s1;
    SL_TRY(scratch(u1 + ".set0", static_cast<size_t>(K1.nk), &d_s1a));
    SL_TRY(scratch(u1 + ".set1", static_cast<size_t>(K1.nk), &d_s1));
    if (K1.nk) {
        hipLaunchKernelGGL(k_keys_to_orig, dim3(nblk(K1.nk, 256)), dim3(256), 0, s, K1.keys, K1.nk, S1.perm, d_s1a);
        SL_TRY(radix_sort_keys(u1 + ".sorttmp", d_s1a, d_s1, static_cast<size_t>(K1.nk), 64, s));
    }
    SortedUmis S2;
    DirectedKeys K2;
    SL_TRY(encode_and_rank(u2, d_c2, d_o2, d_members, d_gid, ngroups, n, &S2, s, d_single, nsingle, max_group));
    SL_TRY(neighbour_keys(u2, S2, limit2, d_single, &K2, s));
    int* d_keep; long long* d_pos;
    SL_TRY(scratch(u2 + ".keep", static_cast<size_t>(K2.nk) + 1, &d_keep));
    SL_TRY(scratch(u2 + ".kpos", static_cast<size_t>(K2.nk) + 1, &d_pos));
    if (K2.nk) hipLaunchKernelGGL(k_intersect_flags, dim3(nblk(K2.nk, 256)), dim3(256), 0, s, K2.keys, K2.nk, S2.perm, d_s1, K1.nk, d_keep);
    SL_HIP(hipMemsetAsync(d_keep + K2.nk, 0, sizeof(int), s));
    SL_TRY(exclusive_scan(u2 + ".scantmp", d_keep, d_pos, static_cast<size_t>(K2.nk) + 1, s));
    long long nkeep = 0;
    SL_HIP(hipMemcpyAsync(&nkeep, d_pos + K2.nk, sizeof nkeep, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    unsigned long long* d_kk;
    SL_TRY(scratch(u2 + ".kept", static_cast<size_t>(nkeep), &d_kk));
    if (K2.nk) hipLaunchKernelGGL(k_compact_keys, dim3(nblk(K2.nk, 256)), dim3(256), 0, s, K2.keys, d_keep, d_pos, K2.nk, d_kk);
    SL_HIP(hipGetLastError());
    return adjacency_from_keys(d_kk, nkeep, S2.perm, n, adj, s);
}

// pairs handed in from outside (the exchange of a tile-sharded search): i < j < n, rank_i << 32 | rank_j
__global__ void k_check_pairs(const unsigned long long* __restrict__ pairs, long long m, unsigned long long n, int* __restrict__ bad) {
    const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const unsigned long long a = pairs[e] >> 32, b = pairs[e] & 0xffffffffull;
    if (a >= n || b >= n || a >= b) *bad = 1;
}

static int upload_strings(UmiWs w, const char* chars, const int64_t* off, int64_t n, uint8_t** d_chars, int64_t** d_off,
                          hipStream_t s) {
    const std::string p = UMI_WS[w];
    const int64_t base = n ? off[0] : 0;
    const int64_t total = n ? off[n] - base : 0;
    std::vector<int64_t> rel(static_cast<size_t>(n) + 1);
    for (int64_t i = 0; i <= n; ++i) rel[i] = (n ? off[i] : 0) - base;
    SL_TRY(upload(p + ".chars", reinterpret_cast<const uint8_t*>(chars) + base, static_cast<size_t>(total), d_chars, s));
    SL_TRY(upload(p + ".off", rel.data(), rel.size(), d_off, s));
    return 0;
}

}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_compute_lev_masked(const char* seq, const int64_t* off, int64_t n, double* out) {
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    if (n < 2) return 0;
    if (n > 60000) return fail("sarlacc_amd: compute_lev_masked is dense (n^2/2 doubles); n = %lld is too large", static_cast<long long>(n));
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    const std::string p = UMI_WS[WS_LEV];
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_LEV, seq, off, n, &d_c, &d_o, s));
    // no ordering needed: encode in input order
    UmiArrays U;
    SL_TRY(alloc_umi(p + ".raw", n, &U));
    unsigned long long *khi, *klo; int *idx, *bad;
    SL_TRY(scratch(p + ".khi", n, &khi));
    SL_TRY(scratch(p + ".klo", n, &klo));
    SL_TRY(scratch(p + ".idx", n, &idx));
    SL_TRY(scratch(p + ".bad", 3, &bad));
    const int init[3] = {std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), 0};
    SL_HIP(hipMemcpyAsync(bad, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_umi_encode, dim3(nblk(n, 256)), dim3(256), 0, s, d_c, d_o, static_cast<const int32_t*>(nullptr), static_cast<int>(n), U, khi, klo, idx, static_cast<const uint8_t*>(nullptr), bad);
    int hbad[3];
    SL_HIP(hipMemcpyAsync(hbad, bad, sizeof hbad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    const bool is_long = hbad[1] != init[1];
    bool xl = false;
    if (is_long) {
        const int maxlen = -hbad[2];
        if (maxlen > UMI_XL_MAX) return fail("sarlacc_amd: sequence longer than %d bases is not supported", UMI_XL_MAX);
        xl = maxlen > UMI_LONG_MAX;
        const int words = xl ? (maxlen + 31) / 32 : UMI_LONG_WORDS, nkeys = (maxlen + UMI_KEY_BASES - 1) / UMI_KEY_BASES;
        SL_TRY(alloc_umi(p + ".rawL", n, &U, words));
        unsigned long long* keys;
        SL_TRY(scratch(p + ".keysL", static_cast<size_t>(n) * nkeys, &keys));
        SL_HIP(hipMemcpyAsync(bad, init, sizeof init, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_umi_encode_long, dim3(nblk(n, 256)), dim3(256), 0, s, d_c, d_o, static_cast<const int32_t*>(nullptr), static_cast<int>(n), U, keys, idx, static_cast<const uint8_t*>(nullptr), bad, words, nkeys);
        SL_HIP(hipMemcpyAsync(hbad, bad, sizeof hbad, hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
    }
    // characters outside ACGTN behave as ordinary distinct letters in the reference
    // (src/compute_lev_masked.cpp:51); only ACGTN is supported here
    if (hbad[0] != init[0]) return fail("sarlacc_amd: sequence contains a character outside ACGTN");
    const long long npairs = n * (n - 1) / 2;
    double* d_out;
    SL_TRY(scratch(p + ".out", static_cast<size_t>(npairs), &d_out));
    if (is_long && xl) hipLaunchKernelGGL(k_lev_dense_long<UMI_XL_MAX>, dim3(nblk(npairs, 128)), dim3(128), 0, s, U, static_cast<int>(n), d_out);
    else if (is_long) hipLaunchKernelGGL(k_lev_dense_long<UMI_LONG_MAX>, dim3(nblk(npairs, 128)), dim3(128), 0, s, U, static_cast<int>(n), d_out);
    else hipLaunchKernelGGL(k_lev_dense, dim3(nblk(npairs, 128)), dim3(128), 0, s, U, static_cast<int>(n), d_out);
    SL_HIP(hipGetLastError());
    SL_HIP(hipMemcpy(out, d_out, sizeof(double) * static_cast<size_t>(npairs), hipMemcpyDeviceToHost));
    return 0;
}

int sarlacc_fast_levdist_test(const char* seq, const int64_t* off, int64_t n, int limit, int64_t* nbr_off,
                              int32_t* nbr, int64_t nbr_cap, int64_t* nbr_need) {
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    *nbr_need = 0;
    nbr_off[0] = 0;
    if (n == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_LV, seq, off, n, &d_c, &d_o, s));
    DevAdj adj;
    SL_TRY(group_adjacency(d_c, d_o, nullptr, nullptr, nullptr, nullptr, nullptr, 1, static_cast<int>(n), limit, limit, &adj, s));
    std::vector<long long> hoff(static_cast<size_t>(n) + 1);
    SL_HIP(hipMemcpy(hoff.data(), adj.off, sizeof(long long) * hoff.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i <= n; ++i) nbr_off[i] = hoff[i];
    *nbr_need = adj.nnz;
    if (!nbr || nbr_cap < adj.nnz) return 0;  // sizing call
    std::vector<int> h(static_cast<size_t>(adj.nnz));
    if (adj.nnz) SL_HIP(hipMemcpy(h.data(), adj.nbr, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
    for (long long i = 0; i < adj.nnz; ++i) nbr[i] = h[i] + 1;
    return 0;
}

int sarlacc_cluster_umis_test(const int64_t* link_off, const int32_t* links, int64_t n, int64_t* nclusters,
                              int64_t* clu_off, int32_t* clu) {
    if (n < 0) return fail("sarlacc_amd: negative number of lists");
    *nclusters = 0;
    clu_off[0] = 0;
    if (n == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    const int64_t nnz = link_off[n] - link_off[0];
    std::vector<long long> hoff(static_cast<size_t>(n) + 1);
    std::vector<int> hn(static_cast<size_t>(nnz) + 1);
    for (int64_t i = 0; i <= n; ++i) hoff[i] = link_off[i] - link_off[0];
    for (int64_t i = 0; i < nnz; ++i) {
        const int32_t v = links[link_off[0] + i];
        if (v < 1 || v > n) return fail("sarlacc_amd: link %d outside 1..%lld", v, static_cast<long long>(n));
        hn[i] = v - 1;
    }
    const std::string p = UMI_WS[WS_ADJ];
    DevAdj adj;
    SL_TRY(upload(p + ".off", hoff.data(), hoff.size(), &adj.off, s));
    SL_TRY(upload(p + ".nbr", hn.data(), hn.size(), &adj.nbr, s));
    adj.nnz = nnz;
    ClusterResult res;
    SL_TRY(cluster_dev(adj, static_cast<int>(n), nullptr, nullptr, 1, true, &res, s));
    std::vector<long long> co(static_cast<size_t>(res.nclu) + 1);
    SL_HIP(hipMemcpy(co.data(), res.d_coff, sizeof(long long) * co.size(), hipMemcpyDeviceToHost));
    if (res.total) SL_HIP(hipMemcpy(clu, res.d_out, sizeof(int32_t) * static_cast<size_t>(res.total), hipMemcpyDeviceToHost));
    for (long long c = 0; c <= res.nclu; ++c) clu_off[c] = co[c];
    *nclusters = res.nclu;
    return 0;
}

int sarlacc_umi_group(const char* umi1, const int64_t* off1, const char* umi2, const int64_t* off2, int64_t n,
                      int thresh1, int thresh2, const int64_t* grp_off, const int32_t* grp, int64_t ngroups,
                      int64_t* nclusters, int64_t* clu_off, int32_t* clu) {
    if (n < 0 || ngroups < 0) return fail("sarlacc_amd: negative sizes");
    *nclusters = 0;
    clu_off[0] = 0;
    if (ngroups == 0) return 0;
    const int64_t total = grp_off[ngroups] - grp_off[0];
    for (int64_t i = 0; i < total; ++i) {
        const int32_t v = grp[grp_off[0] + i];
        if (v < 1 || v > n) return fail("sarlacc_amd: pre-group index %d outside 1..%lld", v, static_cast<long long>(n));
    }
    SL_TRY(ensure_device());
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_in = now();
    hipStream_t s = nullptr;
    uint8_t *d_c1, *d_c2 = nullptr;
    int64_t *d_o1, *d_o2 = nullptr;
    SL_TRY(upload_strings(WS_G1, umi1, off1, n, &d_c1, &d_o1, s));
    if (umi2) SL_TRY(upload_strings(WS_G2, umi2, off2, n, &d_c2, &d_o2, s));
    // all pre-groups go through the kernels together: elements = flattened member list,
    // pairs are only formed inside a pre-group, clusters come back group by group
    if (total > std::numeric_limits<int>::max() - 1024) return fail("sarlacc_amd: more than 2^31 pre-group members");
    const int N = static_cast<int>(total);
    std::vector<int> gid(static_cast<size_t>(N) + 1);
    std::vector<uint8_t> single(static_cast<size_t>(N) + 1, 0);
    int64_t nsingle = 0, max_group = 0;
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t a = grp_off[g] - grp_off[0], b = grp_off[g + 1] - grp_off[0];
        for (int64_t i = a; i < b; ++i) { gid[i] = static_cast<int>(g); single[i] = (b - a == 1); }
        nsingle += (b - a == 1) ? 1 : 0;
        max_group = std::max<int64_t>(max_group, b - a);
    }
    int64_t nc = 0;
    if (N > 0) {
        const std::string g = UMI_WS[WS_G];
        int32_t* d_grp; int* d_gid; uint8_t* d_single;
        SL_TRY(upload(g + ".members", grp + grp_off[0], static_cast<size_t>(N), &d_grp, s));
        SL_TRY(upload(g + ".gid", gid.data(), static_cast<size_t>(N), &d_gid, s));
        SL_TRY(upload(g + ".single", single.data(), static_cast<size_t>(N), &d_single, s));
        DevAdj adj;
        const double t0 = now();
        SL_TRY(group_adjacency(d_c1, d_o1, d_c2, d_o2, d_grp, d_gid, d_single, static_cast<int>(ngroups), N, thresh1, thresh2, &adj, s,
                               static_cast<int>(nsingle), static_cast<int>(max_group)));
        SL_HIP(hipStreamSynchronize(s));
        const double t1 = now();
        ClusterResult res;
        SL_TRY(cluster_dev(adj, N, d_grp, d_gid, static_cast<int>(ngroups), false, &res, s));
        const double t2 = now();
        // where a call's time goes (sarlacc_stage_count): seconds of the neighbour search incl. sorts / of the clustering
        ctx().counts["umi_adjacency_s"] = t1 - t0;
        ctx().counts["umi_cluster_s"] = t2 - t1;
        ctx().counts["umi_links"] = static_cast<double>(adj.nnz);
        std::vector<long long> co(static_cast<size_t>(res.nclu) + 1);
        SL_HIP(hipMemcpy(co.data(), res.d_coff, sizeof(long long) * co.size(), hipMemcpyDeviceToHost));
        if (res.total) SL_HIP(hipMemcpy(clu, res.d_out, sizeof(int32_t) * static_cast<size_t>(res.total), hipMemcpyDeviceToHost));
        for (long long c = 0; c <= res.nclu; ++c) clu_off[c] = co[c];
        nc = res.nclu;
        ctx().counts["umi_tables_in_s"] = t0 - t_in;    // strings and pre-group tables to the device
        ctx().counts["umi_clusters_out_s"] = now() - t2;
    }
    *nclusters = nc;
    return 0;
}

// Row tiles of the all-pairs matrix owned by shard `index` of `count`: boundaries balance the
// triangular work (row tile b meets nt - b column tiles).
static void shard_tiles(int nt, int index, int count, int* lo, int* hi) {
    const double total = 0.5 * nt * (nt + 1.0);
    auto bound = [&](int k) -> int {  // smallest b with work(0..b) >= k/count of the total
        if (k <= 0) return 0;
        if (k >= count) return nt;
        const double want = total * k / count;
        int b = 0;
        double acc = 0;
        while (b < nt && acc < want) { acc += nt - b; ++b; }
        return b;
    };
    *lo = bound(index);
    *hi = bound(index + 1);
}

int sarlacc_umi_pairs_shard(const char* umi, const int64_t* off, int64_t n, int limit, int shard_index,
                            int shard_count, uint64_t* pairs, int64_t cap, int64_t* npairs) {
    if (n < 0 || shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return fail("sarlacc_amd: bad shard request");
    *npairs = 0;
    if (n == 0 || limit < 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_PS, umi, off, n, &d_c, &d_o, s));
    SortedUmis S;
    SL_TRY(encode_and_rank(UMI_WS[WS_U1], d_c, d_o, nullptr, nullptr, 1, static_cast<int>(n), &S, s));
    int lo, hi;
    shard_tiles(static_cast<int>(nblk(n, TILE)), shard_index, shard_count, &lo, &hi);
    unsigned long long* d_edges;
    unsigned long long m;
    g_shard_pairs = -1;
    SL_TRY(pair_edges(UMI_WS[WS_U1], S, limit, lo, hi, &d_edges, &m, s));
    *npairs = static_cast<int64_t>(m);
    if (!pairs || cap < static_cast<int64_t>(m)) return 0;  // sizing call
    if (m) SL_HIP(hipMemcpy(pairs, d_edges, sizeof(uint64_t) * m, hipMemcpyDeviceToHost));
    return 0;
}

// clustering of ONE pre-group from its neighbour pairs, which are already on the device (validated there)
static int group_from_device_pairs(const char* umi, const int64_t* off, int64_t n, int limit, const unsigned long long* d_edges,
                                   int64_t npairs, int64_t* nclusters, int64_t* clu_off, int32_t* clu, hipStream_t s) {
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_PS, umi, off, n, &d_c, &d_o, s));
    SortedUmis S;
    SL_TRY(encode_and_rank(UMI_WS[WS_U1], d_c, d_o, nullptr, nullptr, 1, static_cast<int>(n), &S, s));
    int* d_bad;
    SL_TRY(scratch(std::string(UMI_WS[WS_PS]) + ".badpair", 1, &d_bad));
    SL_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (npairs) hipLaunchKernelGGL(k_check_pairs, dim3(nblk(npairs, 256)), dim3(256), 0, s, d_edges, static_cast<long long>(npairs), static_cast<unsigned long long>(n), d_bad);
    int bad = 0;
    SL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (bad) return fail("sarlacc_amd: malformed neighbour pair");
    const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    DirectedKeys K;
    SL_TRY(keys_from_edges(UMI_WS[WS_U1], S, limit < 0 ? -1 : limit, nullptr, d_edges, static_cast<unsigned long long>(npairs), &K, s));
    DevAdj adj;
    SL_TRY(adjacency_from_keys(K.keys, K.nk, S.perm, static_cast<int>(n), &adj, s));
    SL_HIP(hipStreamSynchronize(s));
    const double t1 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    ClusterResult res;
    SL_TRY(cluster_dev(adj, static_cast<int>(n), nullptr, nullptr, 1, false, &res, s));
    ctx().counts["umi_adjacency_s"] = t1 - t0;
    ctx().counts["umi_cluster_s"] = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t1;
    std::vector<long long> co(static_cast<size_t>(res.nclu) + 1);
    SL_HIP(hipMemcpy(co.data(), res.d_coff, sizeof(long long) * co.size(), hipMemcpyDeviceToHost));
    if (res.total) SL_HIP(hipMemcpy(clu, res.d_out, sizeof(int32_t) * static_cast<size_t>(res.total), hipMemcpyDeviceToHost));
    for (long long c = 0; c <= res.nclu; ++c) clu_off[c] = co[c];
    *nclusters = res.nclu;
    return 0;
}

int sarlacc_umi_group_from_pairs(const char* umi, const int64_t* off, int64_t n, int limit, const uint64_t* pairs,
                                 int64_t npairs, int64_t* nclusters, int64_t* clu_off, int32_t* clu) {
    if (n < 0 || npairs < 0) return fail("sarlacc_amd: negative sizes");
    *nclusters = 0;
    clu_off[0] = 0;
    if (n == 0) return 0;
    if (n == 1) {  // a pre-group of one read passes through (src/umi_group.cpp:39-42)
        clu[0] = 1; clu_off[1] = 1; *nclusters = 1;
        return 0;
    }
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    unsigned long long* d_edges;
    SL_TRY(upload(std::string(UMI_WS[WS_U1]) + ".edges_in", reinterpret_cast<const unsigned long long*>(pairs), static_cast<size_t>(npairs), &d_edges, s));
    return group_from_device_pairs(umi, off, n, limit, d_edges, npairs, nclusters, clu_off, clu, s);
}

// ---- the pair exchange with the pairs kept in HBM (one giant pre-group over several GPUs: 10^8 pairs at 8 x 10^6 reads) ----
int sarlacc_dev_umi_pairs_shard(const char* umi, const int64_t* off, int64_t n, int limit, int shard_index,
                                int shard_count, int64_t* npairs) {
    if (n < 0 || shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return fail("sarlacc_amd: bad shard request");
    *npairs = 0;
    g_shard_pairs = -1;
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    if (n == 0 || limit < 0) { g_shard_pairs = 0; return 0; }
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_PS, umi, off, n, &d_c, &d_o, s));
    SortedUmis S;
    SL_TRY(encode_and_rank(UMI_WS[WS_U1], d_c, d_o, nullptr, nullptr, 1, static_cast<int>(n), &S, s));
    int lo, hi;
    shard_tiles(static_cast<int>(nblk(n, TILE)), shard_index, shard_count, &lo, &hi);
    unsigned long long* d_edges;
    unsigned long long m;
    SL_TRY(pair_edges(UMI_WS[WS_U1], S, limit, lo, hi, &d_edges, &m, s));
    g_shard_pairs = static_cast<long long>(m);   // (they stay in the workspace buffer "u1.edges" until the next search or release)
    *npairs = static_cast<int64_t>(m);
    return 0;
}

int sarlacc_dev_umi_pairs_fetch(uint64_t* d_pairs, int64_t cap) {
    if (g_shard_pairs < 0) return fail("sarlacc_amd: no neighbour pairs to fetch (sarlacc_dev_umi_pairs_shard must be the call before)");
    if (cap < g_shard_pairs) return fail("sarlacc_amd: pair buffer too small (%lld needed)", g_shard_pairs);
    if (g_shard_pairs == 0) return 0;
    auto it = ctx().ws.find(std::string(UMI_WS[WS_U1]) + ".edges");
    if (it == ctx().ws.end() || !it->second.ptr || it->second.cap < sizeof(uint64_t) * static_cast<size_t>(g_shard_pairs)) {
        g_shard_pairs = -1;
        return fail("sarlacc_amd: the neighbour pairs of the last shard search are gone (workspace released)");
    }
    if (!d_pairs) return fail("sarlacc_amd: null pair buffer");
    SL_HIP(hipMemcpy(d_pairs, it->second.ptr, sizeof(uint64_t) * static_cast<size_t>(g_shard_pairs), hipMemcpyDeviceToDevice));
    return 0;
}

int sarlacc_dev_umi_group_from_pairs(const char* umi, const int64_t* off, int64_t n, int limit, const uint64_t* d_pairs,
                                     int64_t npairs, int64_t* nclusters, int64_t* clu_off, int32_t* clu) {
    if (n < 0 || npairs < 0) return fail("sarlacc_amd: negative sizes");
    if (npairs && !d_pairs) return fail("sarlacc_amd: null pair buffer");
    *nclusters = 0;
    clu_off[0] = 0;
    if (n == 0) return 0;
    if (n == 1) {  // a pre-group of one read passes through (src/umi_group.cpp:39-42)
        clu[0] = 1; clu_off[1] = 1; *nclusters = 1;
        return 0;
    }
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    SL_HIP(hipDeviceSynchronize());   // the caller's collective wrote d_pairs on a stream of its own
    return group_from_device_pairs(umi, off, n, limit, reinterpret_cast<const unsigned long long*>(d_pairs), npairs, nclusters, clu_off, clu, s);
}

// Gives back the UMI stage's cached device buffers: every name "<prefix>" or "<prefix>.<what>" of UMI_WS.
int64_t sarlacc_release_umi_workspace(void) {
    return ctx().release_matching([](const std::string& name) {
        for (const char* p : UMI_WS) {
            const size_t n = std::strlen(p);
            if (name.compare(0, n, p) == 0 && (name.size() == n || name[n] == '.')) return true;
        }
        return false;
    });
}
}
