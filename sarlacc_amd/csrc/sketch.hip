// sketch.hip -- reference-free pre-groups of a read batch (generics.sequenceGroups), on gfx950: a one-permutation
// MinHash sketch of every read's k-mers, candidate pairs from equal sketch entries, links between reads that share enough
// of them, connected components of the links.  The host side (sketch_host.cpp) runs the rocPRIM sorts and scans between
// these launches.  The rules are DESIGN §4.19; tests/sketch_cases.py restates them.
//
//   k_sketch        one wavefront per read, 64 bases per step, one byte per lane: coalesced 64-byte loads, those of the next
//                   eight words in flight while a word is hashed (16-byte loads per lane would put 16 consecutive bases
//                   into one lane, and the ballots need base l of a word in lane l).  Four ballots per word (b == 'A', 'C',
//                   'G', 'T'), from which the scalar unit puts the three planes together: low code bit, high code bit,
//                   invalid.  Lane l's k-mer is bits l .. l + k - 1 of the two code planes, taken across the current and the
//                   next word; the reverse complement is ~ and a bit reversal per plane; the k-mer starts without an
//                   invalid base are one 64-bit mask, spread from the invalid plane by shift-or steps on the scalar unit and
//                   used as the execution mask.  No cross-lane traffic besides the ballots.  The bucket minima of the
//                   wavefront live in LDS (8 bytes per bucket, at most 2 KB); a lane reads the slot and issues the 64-bit
//                   atomicMin only when its hash is smaller.
//   k_sk_entry_reads    the read of every sketch entry, the value column of the sort by (hash, read)
//   k_sk_pairs_count / k_sk_pairs_fill   per sorted entry the entries at distance 1 .. window behind it with the same hash
//   k_sk_link_flags / k_sk_link_scatter  over the sorted pair keys: run heads (distinct pairs), heads of runs of at least
//                   min_shared (links: the key min_shared - 1 further on is the same), the links in ascending order
//   k_cc_init / k_cc_hook / k_cc_jump    connected components: a link whose roots differ lowers the larger root to the
//                   smaller by atomicMin, then every vertex is pointed at its root; repeated until a round changes
//                   nothing.  parent[v] <= v always, so the root of a component ends as its lowest vertex whatever the
//                   order of execution.
//   k_cc_heads / k_cc_labels             components numbered in ascending order of their lowest vertex
//
// Memory: a read is loaded only inside [off[r], off[r + 1]), one byte per load, and only after
// 0 <= off[r] <= off[r + 1] <= off[n] has been seen for it (a read that fails is handled as empty and reported), so the
// last read of a buffer of exact size is read like any other.  A link is used only after both ends were seen below n.
// No kernel waits on another workgroup.  A bad value is an error return (SkState), never a trap.
#include "sketch.hpp"

#include "devprim.hpp"

#include <algorithm>

namespace sarlacc {
namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_WAVES = SK_THREADS / 64;
constexpr int SK_AHEAD = 8;      // 64-base words a wavefront has in flight

__device__ __forceinline__ void fence_wave() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// the three planes of 64 bases, bit l from lane l: A = 0, C = 1, G = 2, T = 3, every other byte (and a lane behind the
// read's end, in = false) invalid
struct Planes {
    uint64_t lo, hi, inv;
};

// b: the lane's byte; in: it lies inside the read.  Four compares; the planes are put together on the scalar unit.
__device__ __forceinline__ Planes planes_of(unsigned b, bool in) {
    b = in ? b : 0u;
    const uint64_t a = __builtin_amdgcn_ballot_w64(b == 'A'), c = __builtin_amdgcn_ballot_w64(b == 'C');
    const uint64_t g = __builtin_amdgcn_ballot_w64(b == 'G'), t = __builtin_amdgcn_ballot_w64(b == 'T');
    Planes p;
    p.lo = c | t;
    p.hi = g | t;
    p.inv = ~(a | c | g | t);
    return p;
}

// the same value in every lane, said so to the compiler: what depends on it alone stays in scalar registers
__device__ __forceinline__ long long wave_uniform(long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<int>(v)), hi = __builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32));
    return static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
}

// bit p set: one of the bases p .. p + k - 1 of the 128 in (lo, hi) is invalid.  Scalar work: at most five shift-or steps.
__device__ __forceinline__ uint64_t broken_starts(uint64_t lo, uint64_t hi, int k) {
    for (int cover = 1; cover < k;) {
        const int sh = cover < k - cover ? cover : k - cover;      // 1 .. 16
        lo |= (lo >> sh) | (hi << (64 - sh));
        hi |= hi >> sh;
        cover += sh;
    }
    return lo;
}

// Byte p of a read of len > 0 bytes; behind its end the read's last byte, which the user drops (planes_of(b, p < len)).
// The load is unconditional -- a load inside a branch makes the compiler wait for every load in flight at the next use --
// and nothing is done with its result here, so that it stays in flight.
__device__ __forceinline__ unsigned base_at(const uint8_t* s, long long p, long long len) { return s[p < len ? p : len - 1]; }

// The k-mers that start in the 64 bases of `cur` (lane l: bits l .. l + k - 1 of the planes, the upper ones from `nxt`), hashed
// into the wavefront's bucket minima; returns how many are present.
template <bool CANON>
__device__ __forceinline__ int sketch_word(const Planes& cur, const Planes& nxt, int lane, int k, int hshift, uint64_t* mine) {
    const uint32_t kmask = (1u << k) - 1u;
    const int up = (64 - lane) & 63;                       // (the shift by 64 at lane 0 is masked away)
    const uint64_t take_next = lane ? ~0ull : 0ull;
    const uint32_t lo = static_cast<uint32_t>((cur.lo >> lane) | ((nxt.lo << up) & take_next)) & kmask;
    const uint32_t hi = static_cast<uint32_t>((cur.hi >> lane) | ((nxt.hi << up) & take_next)) & kmask;
    // the lanes whose k bases are all valid: all of them, but for a word with an invalid base in reach (the scalar unit
    // serves the four SIMDs of a CU, so its work is kept off the common path)
    const uint64_t whole = (cur.inv | (nxt.inv & kmask)) ? ~broken_starts(cur.inv, nxt.inv, k) : ~0ull;
    uint64_t x = static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
    if (CANON) {
        const uint32_t rlo = __brev(~lo & kmask) >> (32 - k), rhi = __brev(~hi & kmask) >> (32 - k);
        const uint64_t y = static_cast<uint64_t>(rlo) | (static_cast<uint64_t>(rhi) << 32);
        x = y < x ? y : x;
    }
    const uint64_t h = fmix64(x);
    const uint64_t present = whole & __builtin_amdgcn_ballot_w64(h != SK_EMPTY);
    if (__builtin_amdgcn_inverse_ballot_w64(present)) {
        uint64_t* slot = mine + (h >> hshift);
        if (h < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(reinterpret_cast<unsigned long long*>(slot), h);
    }
    return __popcll(present);
}

template <bool CANON>
__global__ void __launch_bounds__(SK_THREADS) k_sketch(SketchArgs a, uint64_t* sketch, int32_t* nkmers, SkState* st) {
    __shared__ uint64_t minima[SK_WAVES][SK_MAX_BUCKETS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t* mine = minima[wave];
    const int nb = 1 << a.log2_buckets, k = a.k, hshift = 64 - a.log2_buckets;
    const long long total = a.off[a.n];
    const long long nwaves = static_cast<long long>(gridDim.x) * SK_WAVES;
    for (long long r = static_cast<long long>(blockIdx.x) * SK_WAVES + wave; r < a.n; r += nwaves) {
        const long long b0 = wave_uniform(a.off[r]), b1 = wave_uniform(a.off[r + 1]);
        const bool bad = b0 < 0 || b1 < b0 || b1 > total;
        const long long len = bad ? 0 : b1 - b0;
        const uint8_t* s = a.seq + (bad ? 0 : b0);
        for (int j = lane; j < nb; j += 64) mine[j] = SK_EMPTY;
        fence_wave();
        int count = 0;
        if (len >= k) {
            const long long nstart = ((len - k) >> 6) + 1;      // words in which a k-mer starts
            Planes cur = planes_of(base_at(s, lane, len), lane < len);
            // The bytes of the next SK_AHEAD words are on their way while a word is hashed (against one word in flight:
            // 4 % on 2-kb reads).
            unsigned ahead[SK_AHEAD];
#pragma unroll
            for (int i = 0; i < SK_AHEAD; ++i) {
                ahead[i] = base_at(s, ((i + 1) << 6) + lane, len);
            }
            for (long long w0 = 0; w0 < nstart; w0 += SK_AHEAD) {
#pragma unroll
                for (int i = 0; i < SK_AHEAD; ++i) {
                    const Planes nxt = planes_of(ahead[i], ((w0 + i + 1) << 6) + lane < len);
                    ahead[i] = base_at(s, ((w0 + i + 1 + SK_AHEAD) << 6) + lane, len);
                    if (w0 + i < nstart) count += sketch_word<CANON>(cur, nxt, lane, k, hshift, mine);
                    cur = nxt;
                }
            }
        }
        fence_wave();
        uint64_t* out = sketch + (static_cast<size_t>(r) << a.log2_buckets);
        for (int j = lane; j < nb; j += 64) out[j] = mine[j];
        if (lane == 0) {
            nkmers[r] = count;
            if (bad) atomicMin(&st->bad_off, static_cast<unsigned long long>(r));
        }
        fence_wave();
    }
}

__global__ void __launch_bounds__(256) k_sk_entry_reads(long long m, int log2_buckets, int32_t* read) {
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (e < m) read[e] = static_cast<int32_t>(e >> log2_buckets);
}

// entries at distance 1 .. window behind p with p's hash; equal hashes are contiguous, so the first other one ends the walk
__device__ __forceinline__ int same_behind(const uint64_t* hash, long long m, long long p, int window) {
    const uint64_t h = hash[p];
    if (h == SK_EMPTY) return 0;
    int c = 0;
    while (c < window && p + c + 1 < m && hash[p + c + 1] == h) ++c;
    return c;
}

__global__ void __launch_bounds__(256) k_sk_pairs_count(const uint64_t* hash, long long m, int window, int32_t* count) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p > m) return;
    count[p] = p < m ? same_behind(hash, m, p, window) : 0;
}

__global__ void __launch_bounds__(256) k_sk_pairs_fill(const int32_t* read, long long m, const int64_t* begin, int bits, uint64_t* pair) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p >= m) return;
    const int c = static_cast<int>(begin[p + 1] - begin[p]);      // what the count pass saw
    const uint64_t a = static_cast<uint64_t>(static_cast<uint32_t>(read[p])) << bits;
    uint64_t* out = pair + begin[p];
    for (int d = 1; d <= c; ++d) out[d - 1] = a | static_cast<uint32_t>(read[p + d]);
}

__global__ void __launch_bounds__(256) k_sk_link_flags(const uint64_t* pair, long long t, int min_shared, int32_t* flag, SkState* st) {
    __shared__ unsigned long long block_heads;
    if (threadIdx.x == 0) block_heads = 0;
    __syncthreads();
    unsigned long long heads = 0;
    const long long step = static_cast<long long>(gridDim.x) * 256;
    for (long long p = blockIdx.x * 256LL + threadIdx.x; p <= t; p += step) {
        int f = 0;
        if (p < t) {
            const uint64_t key = pair[p];
            if (p == 0 || pair[p - 1] != key) {
                ++heads;
                f = p + min_shared - 1 < t && pair[p + min_shared - 1] == key;
            }
        }
        flag[p] = f;
    }
    if (heads) atomicAdd(&block_heads, heads);
    __syncthreads();
    if (threadIdx.x == 0 && block_heads) atomicAdd(&st->n_pairs, block_heads);
}

__global__ void __launch_bounds__(256) k_sk_link_scatter(const uint64_t* pair, long long t, int bits, const int32_t* flag,
                                                         const int64_t* before, uint64_t* links, long long capacity, SkState* st) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p > t) return;
    if (p == t) { st->n_links = static_cast<unsigned long long>(before[t]); return; }
    if (!flag[p] || !links || before[p] >= capacity) return;
    const uint64_t key = pair[p];
    links[before[p]] = ((key >> bits) << 32) | (key & ((1ull << bits) - 1));
}

// ---- connected components ----
__device__ __forceinline__ int32_t cc_load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ int32_t cc_root(const int32_t* parent, int32_t v) {
    for (int32_t p = cc_load(parent + v); p != v; p = cc_load(parent + v)) v = p;      // parent[v] < v: ends
    return v;
}

__global__ void __launch_bounds__(256) k_cc_init(long long n, int32_t* parent) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v < n) parent[v] = static_cast<int32_t>(v);
}

__global__ void __launch_bounds__(256) k_cc_hook(const uint64_t* links, long long n_links, long long n, const int32_t* nkmers,
                                                 int32_t* parent, SkState* st) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n_links) return;
    const uint64_t link = links[i];
    const long long a = static_cast<long long>(link >> 32), b = static_cast<long long>(link & 0xffffffffull);
    if (a >= n || b >= n) { atomicMin(&st->bad_link, static_cast<unsigned long long>(i)); return; }
    if (nkmers && (nkmers[a] <= 0 || nkmers[b] <= 0)) return;      // such a vertex is in no group
    const int32_t ra = cc_root(parent, static_cast<int32_t>(a)), rb = cc_root(parent, static_cast<int32_t>(b));
    if (ra == rb) return;
    atomicMin(parent + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    st->changed = 1u;
}

// Every vertex halves its own path until its parent is a root; only vertex v's thread writes parent[v], and the roots do
// not move during this kernel.
__global__ void __launch_bounds__(256) k_cc_jump(long long n, int32_t* parent) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v >= n) return;
    for (;;) {
        const int32_t p = cc_load(parent + v), g = cc_load(parent + p);
        if (p == g) break;
        __atomic_store_n(parent + v, g, __ATOMIC_RELAXED);
    }
}

__global__ void __launch_bounds__(256) k_cc_heads(const int32_t* parent, const int32_t* nkmers, long long n, int32_t* head) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v > n) return;
    head[v] = v < n && parent[v] == v && (!nkmers || nkmers[v] > 0);
}

__global__ void __launch_bounds__(256) k_cc_labels(const int32_t* parent, const int32_t* nkmers, long long n, const int32_t* before,
                                                   int32_t* label, SkState* st) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v > n) return;
    if (v == n) { st->n_groups = static_cast<unsigned long long>(before[n]); return; }
    label[v] = (!nkmers || nkmers[v] > 0) ? before[parent[v]] : -1;
}

unsigned capped_grid(long long blocks) {
    return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(blocks, static_cast<long long>(ctx().num_cu) * 16)));
}

}  // namespace

int sk_state_reset(SkState* d_state, hipStream_t s) {
    SL_HIP(hipMemsetAsync(d_state, 0, sizeof(SkState), s));
    SL_HIP(hipMemsetAsync(d_state, 0xff, 2 * sizeof(unsigned long long), s));      // the two bad_*
    return 0;
}

int launch_sketch(const SketchArgs& a, uint64_t* sketch, int32_t* nkmers, SkState* st, hipStream_t s) {
    const dim3 grid(capped_grid(nblk(a.n, SK_WAVES)));
    if (a.canonical) hipLaunchKernelGGL(k_sketch<true>, grid, dim3(SK_THREADS), 0, s, a, sketch, nkmers, st);
    else hipLaunchKernelGGL(k_sketch<false>, grid, dim3(SK_THREADS), 0, s, a, sketch, nkmers, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_sk_entry_reads(long long m, int log2_buckets, int32_t* read, hipStream_t s) {
    hipLaunchKernelGGL(k_sk_entry_reads, dim3(nblk(m, 256)), dim3(256), 0, s, m, log2_buckets, read);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_sk_pairs_count(const uint64_t* hash, long long m, int window, int32_t* count, hipStream_t s) {
    hipLaunchKernelGGL(k_sk_pairs_count, dim3(nblk(m + 1, 256)), dim3(256), 0, s, hash, m, window, count);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_sk_pairs_fill(const int32_t* read, long long m, const int64_t* begin, int bits, uint64_t* pair, hipStream_t s) {
    hipLaunchKernelGGL(k_sk_pairs_fill, dim3(nblk(m, 256)), dim3(256), 0, s, read, m, begin, bits, pair);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_sk_link_flags(const uint64_t* pair, long long t, int min_shared, int32_t* flag, SkState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_sk_link_flags, dim3(capped_grid(nblk(t + 1, 256))), dim3(256), 0, s, pair, t, min_shared, flag, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_sk_link_scatter(const uint64_t* pair, long long t, int bits, const int32_t* flag, const int64_t* before, uint64_t* links,
                           long long capacity, SkState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_sk_link_scatter, dim3(nblk(t + 1, 256)), dim3(256), 0, s, pair, t, bits, flag, before, links, capacity, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_cc_init(long long n, int32_t* parent, hipStream_t s) {
    hipLaunchKernelGGL(k_cc_init, dim3(nblk(n, 256)), dim3(256), 0, s, n, parent);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_cc_hook(const uint64_t* links, long long n_links, long long n, const int32_t* nkmers, int32_t* parent, SkState* st,
                   hipStream_t s) {
    hipLaunchKernelGGL(k_cc_hook, dim3(nblk(n_links, 256)), dim3(256), 0, s, links, n_links, n, nkmers, parent, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_cc_jump(long long n, int32_t* parent, hipStream_t s) {
    hipLaunchKernelGGL(k_cc_jump, dim3(nblk(n, 256)), dim3(256), 0, s, n, parent);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_cc_heads(const int32_t* parent, const int32_t* nkmers, long long n, int32_t* head, hipStream_t s) {
    hipLaunchKernelGGL(k_cc_heads, dim3(nblk(n + 1, 256)), dim3(256), 0, s, parent, nkmers, n, head);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_cc_labels(const int32_t* parent, const int32_t* nkmers, long long n, const int32_t* before, int32_t* label, SkState* st,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_cc_labels, dim3(nblk(n + 1, 256)), dim3(256), 0, s, parent, nkmers, n, before, label, st);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
