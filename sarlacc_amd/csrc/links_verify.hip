// links_verify.hip -- the alignment check of sequenceGroups' links (DESIGN §4.19 rule 6a; sarlacc_dev_links_verify,
// host side in sketch_host.cpp): a link of the sketch stage stays when the banded unit-cost distance of its two reads,
// as they stand or with the second one reverse-complemented, is within the identity threshold.
//
//   k_links_verify    one link per lane, no LDS, no cross-lane traffic: the lane checks the link's ends and the offsets
//                     of its two reads, decides by the lengths alone where it can (||a| - |b|| > min(w, t)), and else
//                     runs lv_banded (links_verify_core.hpp) forward and, if that fails and both strands count, against
//                     the reverse complement.  Either run ends as soon as the distance on the final diagonal passes t.
//                     The band's word count is a template argument (the bandwidth is one per launch).  Out: the
//                     distance (-1: fails), the strand, a flag for the scan.
//   k_links_keep      the passing links to their ranks in input order (the exclusive scan of the flags), and the count
//
// Memory: a read is touched only inside [off[r], off[r + 1]) and only after 0 <= off[r] <= off[r + 1] <= off[n] and a
// length below 2^31 were seen for it; a link only after 0 <= a < b < n.  What fails is reported (SkState), never a trap.
#include "sketch.hpp"

#include "devprim.hpp"
#include "links_verify_core.hpp"

namespace sarlacc {
namespace {

constexpr int LV_THREADS = 256;

template <int NW>
__global__ void __launch_bounds__(LV_THREADS) k_links_verify(VerifyArgs a, int32_t* dist, uint8_t* strand, int32_t* flag, SkState* st) {
    const long long i = blockIdx.x * static_cast<long long>(LV_THREADS) + threadIdx.x;
    if (i > a.n_links) return;
    if (i == a.n_links) { flag[i] = 0; return; }      // the scan's last entry
    const uint64_t link = a.links[i];
    const long long ra = static_cast<long long>(link >> 32), rb = static_cast<long long>(link & 0xffffffffull);
    int d = -1, sd = 0;
    if (!(ra < rb && rb < a.n)) {
        atomicMin(&st->bad_link, static_cast<unsigned long long>(i));
    } else {
        const long long total = a.off[a.n];
        const long long a0 = a.off[ra], a1 = a.off[ra + 1], b0 = a.off[rb], b1 = a.off[rb + 1];
        const bool bad_a = a0 < 0 || a1 < a0 || a1 > total || a1 - a0 > 0x7fffffffLL;
        const bool bad_b = b0 < 0 || b1 < b0 || b1 > total || b1 - b0 > 0x7fffffffLL;
        if (bad_a || bad_b) {
            atomicMin(&st->bad_off, static_cast<unsigned long long>(bad_a ? ra : rb));
        } else {
            const int la = static_cast<int>(a1 - a0), lb = static_cast<int>(b1 - b0);
            const int t = lv_threshold(a.max_diff_ppm, la, lb);
            const int gap = la > lb ? la - lb : lb - la;
            if (gap <= (a.w < t ? a.w : t)) {
                const uint8_t *x = a.seq + a0, *y = a.seq + b0;
#pragma nounroll
                for (int pass = 0; pass < (a.both_strands ? 2 : 1) && d < 0; ++pass) {
                    if (pass) atomicAdd(&st->n_second, 1ull);
                    const int v = lv_banded<NW>(x, la, y, lb, a.w, pass != 0, t);
                    if (v <= t) { d = v; sd = pass; }
                }
            }
        }
    }
    dist[i] = d;
    if (strand) strand[i] = static_cast<uint8_t>(sd);
    flag[i] = d >= 0;
}

__global__ void __launch_bounds__(256) k_links_keep(const uint64_t* links, long long n_links, const int32_t* flag, const int64_t* before,
                                                    uint64_t* kept, SkState* st) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p > n_links) return;
    if (p == n_links) { st->n_kept = static_cast<unsigned long long>(before[n_links]); return; }
    if (flag[p] && kept) kept[before[p]] = links[p];
}

}  // namespace

int launch_links_verify(const VerifyArgs& a, int32_t* dist, uint8_t* strand, int32_t* flag, SkState* st, hipStream_t s) {
    const dim3 grid(nblk(a.n_links + 1, LV_THREADS)), block(LV_THREADS);
    const int rc = pick([&](auto nw) {
        hipLaunchKernelGGL(k_links_verify<decltype(nw)::value>, grid, block, 0, s, a, dist, strand, flag, st);
        return 0;
    }, Ints<1, 2, 4, 7, 8>{}, lv_words(a.w));
    if (rc == NO_KERNEL) return fail("sarlacc_amd: no kernel for a bandwidth of %d", a.w);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_links_keep(const uint64_t* links, long long n_links, const int32_t* flag, const int64_t* before, uint64_t* kept, SkState* st,
                      hipStream_t s) {
    hipLaunchKernelGGL(k_links_keep, dim3(nblk(n_links + 1, 256)), dim3(256), 0, s, links, n_links, flag, before, kept, st);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
