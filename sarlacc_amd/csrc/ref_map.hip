// ref_map.hip -- resident reads assigned to references (generics.referenceGroups; sarlacc_dev_sketch_candidates and
// sarlacc_dev_candidates_assign, host side in ref_map_host.cpp), on gfx950: the sketches of the reads (k_sketch,
// sketch.hip) joined against those of the references, a bounded list of candidates per read, every candidate checked
// by the banded distance of links_verify_core.hpp, one reference chosen.  The rules are DESIGN §4.20 (M2 to M5);
// tests/reference_groups_cases.py restates them.
//
//   k_rm_ref_entries   the reference of every reference-sketch entry, the value column of the sort by (hash, reference);
//                      an entry outside its bucket is reported
//   k_rm_directory     buckets + 1 lower bounds into the sorted hashes: the top bits of a hash are its bucket, so bucket
//                      j's entries are one segment, and the empty entries lie behind the last
//   k_rm_probe_count / k_rm_probe_fill   one read-sketch entry per lane, so a wavefront holds the 64 buckets of a read (or
//                      four reads of 16, or a quarter of a read of 256): a lower bound inside the bucket's segment and the
//                      end of the run that starts there (doubling steps, then a bisection) give the references that hold
//                      the hash, however many; an exclusive scan between the two passes; a hit is the key
//                      read << bits | reference
//   k_rm_select        one read per lane over its stretch of the sorted keys (the fill pass wrote the hits of read r
//                      between begin[r * buckets] and begin[(r + 1) * buckets], and the sort by (read, reference) keeps
//                      them there): a run of equal keys is a reference and its length is `shared`; the lane keeps the
//                      best max_candidates runs by insertion into its own row of the output table
//   k_rm_assign<NW>    one (read, slot) pair per lane, no LDS, no cross-lane traffic: lv_banded with x in the reference
//                      buffer and y in the read buffer, forward and, if that fails and both strands count, against the
//                      reverse complement of the read
//   k_rm_choose        one read per lane over its max_candidates slots
//
// Memory: a sequence is touched only inside [off[i], off[i + 1]) of its own buffer and only after
// 0 <= off[i] <= off[i + 1] <= off[n] and a length below 2^31 were seen for it; a candidate only after it was seen inside
// 0 .. n_refs - 1.  A sorted entry is read only inside [0, m).  What fails is reported (RmState), never a trap.
#include "ref_map.hpp"

#include "devprim.hpp"
#include "links_verify_core.hpp"

namespace sarlacc {
namespace {

constexpr int RM_THREADS = 256;

__global__ void __launch_bounds__(RM_THREADS) k_rm_ref_entries(const uint64_t* sketch, long long m, int log2_buckets, int32_t* ref, RmState* st) {
    const long long e = blockIdx.x * static_cast<long long>(RM_THREADS) + threadIdx.x;
    if (e >= m) return;
    ref[e] = static_cast<int32_t>(e >> log2_buckets);
    const uint64_t h = sketch[e];
    if (h != SK_EMPTY && (h >> (64 - log2_buckets)) != static_cast<uint64_t>(e & ((1 << log2_buckets) - 1)))
        atomicMin(&st->bad_ref_entry, static_cast<unsigned long long>(e));
}

// first p in [lo, hi) with hash[p] >= h (UPPER: > h), hi where there is none
template <bool UPPER>
__device__ __forceinline__ int bound(const uint64_t* hash, int lo, int hi, uint64_t h) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const uint64_t v = hash[mid];
        if (UPPER ? v <= h : v < h) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// first p in [lo, hi) with hash[p] > h, where no entry of [lo, hi) is below h.  Runs are short as a rule and lie beside
// lo, so the end is looked for at lo, lo + 1, lo + 2, lo + 4 ... before the bisection of what is left.
__device__ __forceinline__ int run_end(const uint64_t* hash, int lo, int hi, uint64_t h) {
    int known = lo;                  // [lo, known) holds h
    long long probe = lo;            // (64 bits: lo + the last step may pass 2^31)
    for (long long step = 1; probe < hi && hash[probe] == h; step <<= 1) { known = static_cast<int>(probe) + 1; probe += step; }
    return bound<true>(hash, known, probe < hi ? static_cast<int>(probe) : hi, h);
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_directory(const uint64_t* hash, long long m, int log2_buckets, int32_t* dir) {
    const int j = blockIdx.x * RM_THREADS + threadIdx.x, nb = 1 << log2_buckets;
    if (j > nb) return;
    const uint64_t h = j < nb ? static_cast<uint64_t>(j) << (64 - log2_buckets) : SK_EMPTY;
    dir[j] = bound<false>(hash, 0, static_cast<int>(m), h);
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_probe_count(const uint64_t* read_sketch, long long mr, int log2_buckets, const uint64_t* hash,
                                                               const int32_t* dir, int32_t* first, int32_t* count, RmState* st) {
    const long long e = blockIdx.x * static_cast<long long>(RM_THREADS) + threadIdx.x;
    if (e > mr) return;
    if (e == mr) { count[e] = 0; return; }      // the scan's last entry
    const uint64_t h = read_sketch[e];
    const int j = static_cast<int>(e & ((1 << log2_buckets) - 1));
    int lo = 0, c = 0;
    if (h != SK_EMPTY) {
        if ((h >> (64 - log2_buckets)) != static_cast<uint64_t>(j)) {
            atomicMin(&st->bad_read_entry, static_cast<unsigned long long>(e));
        } else {
            const int seg_end = dir[j + 1];
            lo = bound<false>(hash, dir[j], seg_end, h);
            c = run_end(hash, lo, seg_end, h) - lo;
        }
    }
    first[e] = lo;
    count[e] = c;
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_probe_fill(const int32_t* first, const int64_t* begin, const int32_t* ref, long long mr,
                                                              int log2_buckets, int bits, uint64_t* pair) {
    const long long e = blockIdx.x * static_cast<long long>(RM_THREADS) + threadIdx.x;
    if (e >= mr) return;
    const int c = static_cast<int>(begin[e + 1] - begin[e]);      // what the count pass saw
    const uint64_t r = static_cast<uint64_t>(e >> log2_buckets) << bits;
    const int32_t* from = ref + first[e];
    uint64_t* out = pair + begin[e];
    for (int d = 0; d < c; ++d) out[d] = r | static_cast<uint32_t>(from[d]);
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_select(const uint64_t* pair, const int64_t* begin, long long n_reads, int log2_buckets,
                                                          int bits, int min_shared, int k, int32_t* cand_ref, int32_t* cand_shared,
                                                          int32_t* ncand) {
    const long long r = blockIdx.x * static_cast<long long>(RM_THREADS) + threadIdx.x;
    if (r >= n_reads) return;
    int32_t* ref_row = cand_ref + r * k;
    int32_t* shared_row = cand_shared + r * k;      // descending; among equals in the order of arrival, which is by reference
    for (int s = 0; s < k; ++s) { ref_row[s] = -1; shared_row[s] = 0; }
    int n = 0;
    const long long p1 = begin ? begin[(r + 1) << log2_buckets] : 0;
    for (long long p = begin ? begin[r << log2_buckets] : 0; p < p1;) {
        const uint64_t key = pair[p];
        long long q = p + 1;
        while (q < p1 && pair[q] == key) ++q;
        const int shared = static_cast<int>(q - p);
        p = q;
        if (shared < min_shared || (n == k && shared <= shared_row[k - 1])) continue;
        int at = n < k ? n++ : k - 1;
        for (; at > 0 && shared_row[at - 1] < shared; --at) { ref_row[at] = ref_row[at - 1]; shared_row[at] = shared_row[at - 1]; }
        ref_row[at] = static_cast<int32_t>(key & ((1ull << bits) - 1));
        shared_row[at] = shared;
    }
    ncand[r] = n;
}

__device__ __forceinline__ bool bad_span(long long b0, long long b1, long long total) {
    return b0 < 0 || b1 < b0 || b1 > total || b1 - b0 > 0x7fffffffLL;
}

template <int NW>
__global__ void __launch_bounds__(RM_THREADS) k_rm_assign(AssignArgs a, int32_t* cand_dist, uint8_t* cand_strand, RmState* st) {
    const long long i = blockIdx.x * static_cast<long long>(RM_THREADS) + threadIdx.x;
    if (i >= a.n_reads * a.k) return;
    const long long r = i / a.k, f = a.cand_ref[i];
    int d = -1, sd = 0;
    if (f < -1 || f >= a.n_refs) {
        atomicMin(&st->bad_cand, static_cast<unsigned long long>(r));
    } else if (f >= 0) {
        const long long x0 = a.ref_off[f], x1 = a.ref_off[f + 1], y0 = a.read_off[r], y1 = a.read_off[r + 1];
        const bool bad_x = bad_span(x0, x1, a.ref_off[a.n_refs]), bad_y = bad_span(y0, y1, a.read_off[a.n_reads]);
        if (bad_x) atomicMin(&st->bad_ref, static_cast<unsigned long long>(f));
        if (bad_y) atomicMin(&st->bad_read, static_cast<unsigned long long>(r));
        if (!bad_x && !bad_y) {
            atomicAdd(&st->n_checked, 1ull);
            const int lx = static_cast<int>(x1 - x0), ly = static_cast<int>(y1 - y0);
            const int t = lv_threshold(a.max_diff_ppm, lx, ly);
            const int gap = lx > ly ? lx - ly : ly - lx;
            if (gap <= (a.w < t ? a.w : t)) {
                const uint8_t *x = a.ref_seq + x0, *y = a.read_seq + y0;
#pragma nounroll
                for (int pass = 0; pass < (a.both_strands ? 2 : 1) && d < 0; ++pass) {
                    if (pass) atomicAdd(&st->n_second, 1ull);
                    const int v = lv_banded<NW>(x, lx, y, ly, a.w, pass != 0, t);
                    if (v <= t) { d = v; sd = pass; }
                }
            }
        }
    }
    cand_dist[i] = d;
    cand_strand[i] = static_cast<uint8_t>(sd);
}

template <bool CHECK>
__global__ void __launch_bounds__(RM_THREADS) k_rm_choose(AssignArgs a, const int32_t* cand_shared, int32_t* cand_dist, uint8_t* cand_strand,
                                                          int32_t* reference, uint8_t* strand, int32_t* dist, int32_t* shared, RmState* st) {
    const long long r = blockIdx.x * static_cast<long long>(RM_THREADS) + threadIdx.x;
    if (r >= a.n_reads) return;
    const long long row = r * a.k;
    int best = -1, d = -1;
    if (CHECK) {
        for (int s = 0; s < a.k; ++s) {
            const int v = cand_dist[row + s];
            if (v >= 0 && (best < 0 || v < d)) { best = s; d = v; }
        }
    } else {
        bool bad = false;
        for (int s = 0; s < a.k; ++s) {
            const long long f = a.cand_ref[row + s];
            bad |= f < -1 || f >= a.n_refs;
            if (cand_dist) cand_dist[row + s] = -1;
            if (cand_strand) cand_strand[row + s] = 0;
        }
        if (bad) atomicMin(&st->bad_cand, static_cast<unsigned long long>(r));
        else if (a.cand_ref[row] >= 0) best = 0;
    }
    reference[r] = best < 0 ? -1 : a.cand_ref[row + best];
    strand[r] = CHECK && best >= 0 ? cand_strand[row + best] : 0;
    dist[r] = d;
    shared[r] = best < 0 ? 0 : cand_shared[row + best];
}

}  // namespace

int rm_state_reset(RmState* d_state, hipStream_t s) {
    SL_HIP(hipMemsetAsync(d_state, 0, sizeof(RmState), s));
    SL_HIP(hipMemsetAsync(d_state, 0xff, 5 * sizeof(unsigned long long), s));      // the five bad_*
    return 0;
}

int launch_rm_ref_entries(const uint64_t* sketch, long long m, int log2_buckets, int32_t* ref, RmState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_rm_ref_entries, dim3(nblk(m, RM_THREADS)), dim3(RM_THREADS), 0, s, sketch, m, log2_buckets, ref, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_rm_directory(const uint64_t* hash, long long m, int log2_buckets, int32_t* dir, hipStream_t s) {
    hipLaunchKernelGGL(k_rm_directory, dim3(nblk((1 << log2_buckets) + 1, RM_THREADS)), dim3(RM_THREADS), 0, s, hash, m, log2_buckets, dir);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_rm_probe_count(const uint64_t* read_sketch, long long mr, int log2_buckets, const uint64_t* hash, const int32_t* dir,
                          int32_t* first, int32_t* count, RmState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_rm_probe_count, dim3(nblk(mr + 1, RM_THREADS)), dim3(RM_THREADS), 0, s, read_sketch, mr, log2_buckets, hash, dir,
                       first, count, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_rm_probe_fill(const int32_t* first, const int64_t* begin, const int32_t* ref, long long mr, int log2_buckets, int bits,
                         uint64_t* pair, hipStream_t s) {
    hipLaunchKernelGGL(k_rm_probe_fill, dim3(nblk(mr, RM_THREADS)), dim3(RM_THREADS), 0, s, first, begin, ref, mr, log2_buckets, bits, pair);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_rm_select(const uint64_t* pair, const int64_t* begin, long long n_reads, int log2_buckets, int bits, int min_shared, int k,
                     int32_t* cand_ref, int32_t* cand_shared, int32_t* ncand, hipStream_t s) {
    hipLaunchKernelGGL(k_rm_select, dim3(nblk(n_reads, RM_THREADS)), dim3(RM_THREADS), 0, s, pair, begin, n_reads, log2_buckets, bits,
                       min_shared, k, cand_ref, cand_shared, ncand);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_rm_assign(const AssignArgs& a, int32_t* cand_dist, uint8_t* cand_strand, RmState* st, hipStream_t s) {
    const dim3 grid(nblk(a.n_reads * a.k, RM_THREADS)), block(RM_THREADS);
    const int rc = pick([&](auto nw) {
        hipLaunchKernelGGL(k_rm_assign<decltype(nw)::value>, grid, block, 0, s, a, cand_dist, cand_strand, st);
        return 0;
    }, Ints<1, 2, 4, 7, 8>{}, lv_words(a.w));
    if (rc == NO_KERNEL) return fail("sarlacc_amd: no kernel for a bandwidth of %d", a.w);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_rm_choose(const AssignArgs& a, int check, const int32_t* cand_shared, int32_t* cand_dist, uint8_t* cand_strand,
                     int32_t* reference, uint8_t* strand, int32_t* dist, int32_t* shared, RmState* st, hipStream_t s) {
    const dim3 grid(nblk(a.n_reads, RM_THREADS)), block(RM_THREADS);
    if (check) hipLaunchKernelGGL(k_rm_choose<true>, grid, block, 0, s, a, cand_shared, cand_dist, cand_strand, reference, strand, dist, shared, st);
    else hipLaunchKernelGGL(k_rm_choose<false>, grid, block, 0, s, a, cand_shared, cand_dist, cand_strand, reference, strand, dist, shared, st);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
