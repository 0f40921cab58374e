// umi.hip -- the UMI stage's adjacency and dense distances on gfx950: kernels and the device steps that enqueue them.
// Directed adjacency is a radix sort of (row << 32 | column-rank) keys of the undirected pairs of the search
// (umi_search.hip); the greedy clustering is in umi_cluster.hip; the entry points (compute_lev_masked, the reference's
// src/compute_lev_masked.cpp:13-64, and the per pre-group driver umi_group, src/umi_group.cpp:14-116) and everything that
// decides in umi_host.cpp.  Design: DESIGN.md "UMI stage".
#include "umi_common.hpp"

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

// pairs handed in from outside (the exchange of a tile-sharded search): i < j < n, rank_i << 32 | rank_j
__global__ void k_check_pairs(const unsigned long long* __restrict__ pairs, long long m, unsigned long long n, int* __restrict__ bad) {
    const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const unsigned long long a = pairs[e] >> 32, b = pairs[e] & 0xffffffffull;
    if (a >= n || b >= n || a >= b) *bad = 1;
}

// ---------------------------------------------------------------------------
// device steps (umi_common.hpp)

// Which ranks get a self link, and where among the keys; self->n: how many.
int self_links(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single, SelfLinks* out, hipStream_t s) {
    const int n = S.n;
    SL_TRY(scratch(p + ".sflag", static_cast<size_t>(n) + 1, &out->flag));
    SL_TRY(scratch(p + ".spos", static_cast<size_t>(n) + 1, &out->pos));
    hipLaunchKernelGGL(k_self_flags, dim3(nblk(n, 256)), dim3(256), 0, s, S.U, n, 2 * limit, d_single, S.perm, out->flag);
    SL_HIP(hipMemsetAsync(out->flag + n, 0, sizeof(int), s));
    SL_TRY(exclusive_scan(p + ".scantmp", out->flag, out->pos, static_cast<size_t>(n) + 1, s));
    out->n = 0;
    SL_HIP(hipMemcpyAsync(&out->n, out->pos + n, sizeof out->n, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

// Directed, sorted adjacency keys (self links included) from undirected rank pairs.
int directed_keys(const std::string& p, const SortedUmis& S, const unsigned long long* d_edges, unsigned long long m,
                  const SelfLinks& self, DirectedKeys* out, hipStream_t s) {
    const int n = S.n;
    const long long nk = 2 * static_cast<long long>(m) + self.n;
    unsigned long long *d_k0, *d_k1;
    SL_TRY(scratch(p + ".k0", static_cast<size_t>(nk), &d_k0));
    SL_TRY(scratch(p + ".k1", static_cast<size_t>(nk), &d_k1));
    if (m) hipLaunchKernelGGL(k_expand_edges, dim3(nblk(static_cast<long long>(m), 256)), dim3(256), 0, s, d_edges, m, S.perm, d_k0 + self.n);
    hipLaunchKernelGGL(k_self_keys, dim3(nblk(n, 256)), dim3(256), 0, s, self.flag, self.pos, S.perm, n, d_k0);
    SL_HIP(hipGetLastError());
    if (nk) SL_TRY(radix_sort_keys(p + ".sorttmp", d_k0, d_k1, static_cast<size_t>(nk), 32 + ceil_log2(static_cast<unsigned long long>(n) + 1), s));
    out->keys = d_k1;
    out->nk = nk;
    return 0;
}

int adjacency_from_keys(const unsigned long long* keys, long long nk, const int* perm, int n, DevAdj* adj, hipStream_t s) {
    const std::string p = UMI_WS[WS_ADJ];
    SL_TRY(scratch(p + ".off", static_cast<size_t>(n) + 1, &adj->off));
    SL_TRY(scratch(p + ".nbr", static_cast<size_t>(nk), &adj->nbr));
    hipLaunchKernelGGL(k_row_offsets, dim3(nblk(nk + 1, 256)), dim3(256), 0, s, keys, nk, n, adj->off);
    if (nk) hipLaunchKernelGGL(k_cols_from_keys, dim3(nblk(nk, 256)), dim3(256), 0, s, keys, nk, perm, adj->nbr);
    SL_HIP(hipGetLastError());
    adj->nnz = nk;
    return 0;
}

// membership set of one UMI's links keyed by original column id, sorted
int link_set(const std::string& p, const DirectedKeys& K, const int* perm, unsigned long long** d_set, hipStream_t s) {
    unsigned long long* d_s1a;
    SL_TRY(scratch(p + ".set0", static_cast<size_t>(K.nk), &d_s1a));
    SL_TRY(scratch(p + ".set1", static_cast<size_t>(K.nk), d_set));
    if (K.nk) {
        hipLaunchKernelGGL(k_keys_to_orig, dim3(nblk(K.nk, 256)), dim3(256), 0, s, K.keys, K.nk, perm, d_s1a);
        SL_TRY(radix_sort_keys(p + ".sorttmp", d_s1a, *d_set, static_cast<size_t>(K.nk), 64, s));
    }
    return 0;
}

// the links of K that are in the set, in K's order
int links_in_set(const std::string& p, const DirectedKeys& K, const int* perm, const unsigned long long* d_set, long long nset,
                 DirectedKeys* kept, hipStream_t s) {
    int* d_keep; long long* d_pos;
    SL_TRY(scratch(p + ".keep", static_cast<size_t>(K.nk) + 1, &d_keep));
    SL_TRY(scratch(p + ".kpos", static_cast<size_t>(K.nk) + 1, &d_pos));
    if (K.nk) hipLaunchKernelGGL(k_intersect_flags, dim3(nblk(K.nk, 256)), dim3(256), 0, s, K.keys, K.nk, perm, d_set, nset, d_keep);
    SL_HIP(hipMemsetAsync(d_keep + K.nk, 0, sizeof(int), s));
    SL_TRY(exclusive_scan(p + ".scantmp", d_keep, d_pos, static_cast<size_t>(K.nk) + 1, s));
    kept->nk = 0;
    SL_HIP(hipMemcpyAsync(&kept->nk, d_pos + K.nk, sizeof kept->nk, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    SL_TRY(scratch(p + ".kept", static_cast<size_t>(kept->nk), &kept->keys));
    if (K.nk) hipLaunchKernelGGL(k_compact_keys, dim3(nblk(K.nk, 256)), dim3(256), 0, s, K.keys, d_keep, d_pos, K.nk, kept->keys);
    SL_HIP(hipGetLastError());
    return 0;
}

// *bad: some pair is not i < j < n
int check_pairs(const unsigned long long* d_edges, long long npairs, long long n, int* bad, hipStream_t s) {
    int* d_bad;
    SL_TRY(scratch(std::string(UMI_WS[WS_PS]) + ".badpair", 1, &d_bad));
    SL_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (npairs) hipLaunchKernelGGL(k_check_pairs, dim3(nblk(npairs, 256)), dim3(256), 0, s, d_edges, npairs, static_cast<unsigned long long>(n), d_bad);
    *bad = 0;
    SL_HIP(hipMemcpyAsync(bad, d_bad, sizeof *bad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

// every pair's distance, at the encode's word class
int dense_distances(const std::string& p, const UmiArrays& U, int n, int words, double** d_out, hipStream_t s) {
    const long long npairs = static_cast<long long>(n) * (n - 1) / 2;
    SL_TRY(scratch(p + ".out", static_cast<size_t>(npairs), d_out));
    if (words > UMI_LONG_WORDS) hipLaunchKernelGGL(k_lev_dense_long<UMI_XL_MAX>, dim3(nblk(npairs, 128)), dim3(128), 0, s, U, n, *d_out);
    else if (words > 1) hipLaunchKernelGGL(k_lev_dense_long<UMI_LONG_MAX>, dim3(nblk(npairs, 128)), dim3(128), 0, s, U, n, *d_out);
    else hipLaunchKernelGGL(k_lev_dense, dim3(nblk(npairs, 128)), dim3(128), 0, s, U, n, *d_out);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
