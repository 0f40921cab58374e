// umi_cluster.hip -- greedy UMI clustering on gfx950.
// Replaces cluster_umis (the reference's src/cluster_umis.cpp:7-112).  The greedy clustering is
// sequential by definition; it is evaluated exactly, in parallel rounds: a node whose (remaining, index) key is the
// maximum within two hops cannot be affected by any earlier pick, so all such nodes are picked in the same round.
// The pick sequence of the reference is recovered by sorting the picks by their key (descending), solos first
// (SURVEY section 0, App.B Q12).  This file: the kernels and one device step per round kind; the round control is
// cluster_dev (umi_host.cpp).  Design: DESIGN.md "UMI stage".
#include "umi_common.hpp"

namespace sarlacc {

// ---------------------------------------------------------------------------
// greedy clustering in exact parallel rounds

// (ClusterState, ClusterTop and the control block's names: umi_common.hpp)

__global__ void k_cl_init(ClusterState S, int check_sym) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n) return;
    const long long a = S.off[v], b = S.off[v + 1];
    const int deg = static_cast<int>(b - a);
    S.remaining[v] = deg;
    S.seed[v] = 0; S.csize[v] = 0; S.mark[v] = -1; S.pickkey[v] = 0;
    int st = 0;
    if (deg == 0) { atomicMin(&S.err[0], v); st = 1; }
    else if (deg == 1) {
        if (S.nbr[a] != v) atomicMin(&S.err[1], v);
        st = 1;
    } else if (check_sym) {
        bool self = false;
        for (long long p = a; p < b; ++p) {
            const int w = S.nbr[p];
            if (w == v) self = true;
            else {  // symmetric?
                bool back = false;
                for (long long q = S.off[w]; q < S.off[w + 1] && !back; ++q) back = S.nbr[q] == v;
                if (!back) atomicMin(&S.err[2], v);
            }
        }
        if (!self) atomicMin(&S.err[2], v);
        // a node named twice would be stored twice in memb: a cluster list of more than n entries
        bool twice = false;
        for (long long p = a + 1; p < b && !twice; ++p)
            for (long long q = a; q < p && !twice; ++q) twice = S.nbr[q] == S.nbr[p];
        if (twice) atomicMin(&S.err[3], v);
    }
    S.state[v] = st;
}

__global__ void k_cl_keys(ClusterState S) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n) return;
    unsigned long long k = 0;
    if (S.state[v] == 0 && S.remaining[v] > 0) {
        k = (static_cast<unsigned long long>(S.remaining[v]) << 32) | static_cast<unsigned>(v);
        atomicAdd(S.live, 1);
    }
    S.key[v] = k;
}

__global__ void k_cl_m1(ClusterState S) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n) return;
    unsigned long long m = 0;
    if (S.state[v] == 0)
        for (long long p = S.off[v]; p < S.off[v + 1]; ++p) m = max(m, S.key[S.nbr[p]]);
    S.m1[v] = m;
}

// A live node is picked when its key is the maximum over everything within two hops
// through live nodes: no earlier pick of the sequential greedy can touch it.
__global__ void k_cl_pick(ClusterState S, int round) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n) return;
    const unsigned long long k = S.key[v];
    if (k == 0) return;
    unsigned long long m2 = k;
    for (long long p = S.off[v]; p < S.off[v + 1]; ++p) {
        const int w = S.nbr[p];
        if (S.state[w] == 0) m2 = max(m2, S.m1[w]);
    }
    if (m2 != k) return;
    // cluster = still-unused neighbours in list order (src/cluster_umis.cpp:78-91)
    int c = 0;
    const long long a = S.off[v];
    for (long long p = a; p < S.off[v + 1]; ++p) {
        const int w = S.nbr[p];
        if (S.state[w] == 0) { S.memb[a + c] = w; ++c; S.mark[w] = round; }
    }
    S.csize[v] = c;
    S.seed[v] = 1;
    S.pickkey[v] = k;
}

// The same three passes with one wavefront per node, for dense neighbourhoods (threshold 3 on 12-base UMIs: hundreds
// of neighbours per node, thousands for some -- one thread per node would walk them alone): the lanes stride over the
// node's list, so the list is read coalesced and the neighbours' words are gathered 64 at a time.
__device__ __forceinline__ unsigned long long cl_wave_max64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = static_cast<unsigned>(__shfl_xor(static_cast<int>(v), d));
        const unsigned hi = static_cast<unsigned>(__shfl_xor(static_cast<int>(v >> 32), d));
        const unsigned long long o = (static_cast<unsigned long long>(hi) << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(256) k_cl_m1_w(ClusterState S) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= S.n) return;
    unsigned long long m = 0;
    if (S.state[v] == 0)
        for (long long p = S.off[v] + lane; p < S.off[v + 1]; p += 64) m = max(m, S.key[S.nbr[p]]);
    m = cl_wave_max64(m);
    if (lane == 0) S.m1[v] = m;
}

__global__ void __launch_bounds__(256) k_cl_pick_w(ClusterState S, int round) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= S.n) return;
    const unsigned long long k = S.key[v];
    if (k == 0) return;
    const long long a = S.off[v], b = S.off[v + 1];
    unsigned long long m2 = k;
    for (long long p = a + lane; p < b; p += 64) {
        const int w = S.nbr[p];
        if (S.state[w] == 0) m2 = max(m2, S.m1[w]);
    }
    m2 = cl_wave_max64(m2);
    if (m2 != k) return;
    // cluster = still-unused neighbours in list order (src/cluster_umis.cpp:78-91)
    int c = 0;
    for (long long p0 = a; p0 < b; p0 += 64) {
        const long long p = p0 + lane;
        const int w = p < b ? S.nbr[p] : -1;
        const bool live = w >= 0 && S.state[w] == 0;
        const unsigned long long ball = __ballot(live);
        if (live) {
            S.memb[a + c + __popcll(ball & ((1ull << lane) - 1ull))] = w;
            S.mark[w] = round;
        }
        c += __popcll(ball);
    }
    if (lane == 0) { S.csize[v] = c; S.seed[v] = 1; S.pickkey[v] = k; }
}

__global__ void __launch_bounds__(256) k_cl_decrement_w(ClusterState S, int round) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= S.n || S.mark[v] != round) return;
    for (long long p = S.off[v] + lane; p < S.off[v + 1]; p += 64) {
        const int x = S.nbr[p];
        if (S.state[x] == 0) atomicSub(&S.remaining[x], 1);
    }
}

// Dense graphs (threshold 3 on 12-base UMIs: the 2-hop ball of a node covers a large share of the graph) yield only a
// few picks per round, all of them among the nodes with the largest keys, while the two passes above walk every live
// list.  A round can instead be decided on a candidate set C = {live v : remaining[v] >= t}: C is closed upwards in key
// order, so a candidate is a 2-hop maximum of the whole graph exactly when no other CANDIDATE with a larger key lies
// within two hops -- hop1[w] = max key over candidates adjacent to w (lists are symmetric), and v is picked iff the
// maximum of hop1 over its live neighbours is its own key.  Picks outside C are left for a later round (every pick is
// valid on its own), so the clusters are those of the full rounds; the work per round is |C| lists instead of all.
// Control block of the candidate-set rounds.  The decisions between two rounds -- is anything left, did the last candidate
// list overflow, how wide is the next one -- need three counters of the round before; taken on the host they cost one
// read-back per round (190 us per round with its six launches, 330 rounds at threshold 3 on 10^6 12-base UMIs).  k_cl_control
// takes them on the device, every kernel of a round looks at the mode first, and the host enqueues CL_GROUP rounds at a time.

__global__ void __launch_bounds__(1024) k_cl_keys_top(ClusterState S, ClusterTop T) {
    __shared__ int s_live[16], s_max[16];
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    int rem = 0;
    if (v < S.n && S.state[v] == 0 && S.remaining[v] > 0) rem = S.remaining[v];
    if (v < S.n) {
        S.key[v] = rem ? ((static_cast<unsigned long long>(rem) << 32) | static_cast<unsigned>(v)) : 0ull;
        if (T.ctl) T.hop1[v] = 0ull;   // (device-controlled rounds: the round's maxima start here instead of in a memset)
    }
    const unsigned long long live = __ballot(rem > 0);
    int m = rem;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) { s_live[threadIdx.x >> 6] = __popcll(live); s_max[threadIdx.x >> 6] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nl = 0, mm = 0;
        for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) { nl += s_live[w]; mm = max(mm, s_max[w]); }
        if (nl) { atomicAdd(S.live, nl); atomicMax(T.maxrem, mm); }
    }
}

// One thread between the key pass and the candidate pass of a round: the host loop's decisions (see ClusterTop).
__global__ void k_cl_control(ClusterState S, ClusterTop T) {
    int* const c = T.ctl;
    const int live = *S.live;
    c[CTL_MAXREM] = *T.maxrem;
    *S.live = 0; *T.maxrem = 0;
    if (c[CTL_MODE] != CL_TOP) return;   // finished, or waiting for the host's round over every list
    if (live == 0) { c[CTL_MODE] = CL_DONE; return; }
    int delta = c[CTL_DELTA];
    if (c[CTL_WAS_TOP]) {
        // the candidate list of the previous round: cut off -> a round over every list and the window shrinks;
        // a productive list (a quarter or more of it picked) may be hiding picks just below it -> widen
        const long long nc = T.counts[0], np = T.counts[1];
        if (T.counts[2]) { c[CTL_DELTA] = delta / 2; c[CTL_MODE] = CL_WANTS_FULL; c[CTL_WAS_TOP] = 0; return; }
        if (4 * np >= nc) { delta = 2 * delta + 1; c[CTL_WIDENED] += 1; }
        else if (64 * np < nc && nc > 256) { delta /= 2; c[CTL_NARROWED] += 1; }
    }
    c[CTL_DELTA] = delta; c[CTL_WAS_TOP] = 1; c[CTL_ROUNDS] += 1;
    T.counts[0] = T.counts[1] = T.counts[2] = T.counts[3] = 0;
}

__global__ void k_cl_collect(ClusterState S, ClusterTop T, int delta) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (T.ctl && T.ctl[CTL_MODE] != CL_TOP) return;
    const int t = T.ctl ? max(1, T.ctl[CTL_MAXREM] - T.ctl[CTL_DELTA]) : max(1, *T.maxrem - delta);
    const bool in = v < S.n && static_cast<int>(S.key[v] >> 32) >= t;
    const unsigned long long ball = __ballot(in);
    if (!ball) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(&T.counts[0], __popcll(ball));
    base = __shfl(base, 0);
    if (in) {
        const int slot = base + __popcll(ball & ((1ull << lane) - 1ull));
        if (slot < T.cap) T.cand[slot] = v; else atomicExch(&T.counts[2], 1);
    }
}

__global__ void __launch_bounds__(256) k_cl_mark_top(ClusterState S, ClusterTop T) {
    if (T.ctl && T.ctl[CTL_MODE] != CL_TOP) return;
    if (T.counts[2]) return;
    const int nc = T.counts[0], lane = threadIdx.x & 63;
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < nc; c += gridDim.x * 4) {
        const int v = T.cand[c];
        const unsigned long long k = S.key[v];
        for (long long p = S.off[v] + lane; p < S.off[v + 1]; p += 64) {
            const int w = S.nbr[p];
            if (S.state[w] == 0) atomicMax(&T.hop1[w], k);
        }
    }
}

__global__ void __launch_bounds__(256) k_cl_pick_top(ClusterState S, ClusterTop T, int round) {
    if (T.ctl && T.ctl[CTL_MODE] != CL_TOP) return;
    if (T.counts[2]) return;
    const int nc = T.counts[0], lane = threadIdx.x & 63;
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < nc; c += gridDim.x * 4) {
        const int v = T.cand[c];
        const unsigned long long k = S.key[v];
        const long long a = S.off[v], b = S.off[v + 1];
        unsigned long long m2 = k;
        for (long long p = a + lane; p < b; p += 64) {
            const int w = S.nbr[p];
            if (S.state[w] == 0) m2 = max(m2, T.hop1[w]);
        }
        m2 = cl_wave_max64(m2);
        if (m2 != k) continue;
        // cluster = still-unused neighbours in list order (src/cluster_umis.cpp:78-91)
        int cnt = 0;
        for (long long p0 = a; p0 < b; p0 += 64) {
            const long long p = p0 + lane;
            const int w = p < b ? S.nbr[p] : -1;
            const bool live = w >= 0 && S.state[w] == 0;
            const unsigned long long ball = __ballot(live);
            int lbase = 0;
            if (T.marked && ball) {
                if (lane == 0) lbase = atomicAdd(&T.counts[3], __popcll(ball));
                lbase = __shfl(lbase, 0);
            }
            if (live) {
                const int before = __popcll(ball & ((1ull << lane) - 1ull));
                S.memb[a + cnt + before] = w;
                S.mark[w] = round;
                if (T.marked) T.marked[lbase + before] = w;
            }
            cnt += __popcll(ball);
        }
        if (lane == 0) { S.csize[v] = cnt; S.seed[v] = 1; S.pickkey[v] = k; atomicAdd(&T.counts[1], 1); }
    }
}

// commit and decrement of a device-controlled round, over the list of the nodes it clustered instead of over all nodes
__global__ void __launch_bounds__(256) k_cl_commit_list(ClusterState S, ClusterTop T) {
    if (T.ctl[CTL_MODE] != CL_TOP) return;
    const int nm = T.counts[3];
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nm; q += gridDim.x * blockDim.x) {
        const int w = T.marked[q];
        S.state[w] = 2; S.remaining[w] = 0;
    }
}

__global__ void __launch_bounds__(256) k_cl_decrement_list(ClusterState S, ClusterTop T) {
    if (T.ctl[CTL_MODE] != CL_TOP) return;
    const int nm = T.counts[3], lane = threadIdx.x & 63;
    for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < nm; q += gridDim.x * 4) {
        const int v = T.marked[q];
        for (long long p = S.off[v] + lane; p < S.off[v + 1]; p += 64) {
            const int x = S.nbr[p];
            if (S.state[x] == 0) atomicSub(&S.remaining[x], 1);
        }
    }
}

// state flips happen in a separate pass so that k_cl_pick sees a consistent snapshot
__global__ void k_cl_commit(ClusterState S, int round) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n) return;
    if (S.mark[v] == round) { S.state[v] = 2; S.remaining[v] = 0; }
}

__global__ void k_cl_decrement(ClusterState S, int round) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n || S.mark[v] != round) return;
    for (long long p = S.off[v]; p < S.off[v + 1]; ++p) {
        const int x = S.nbr[p];
        if (S.state[x] == 0) atomicSub(&S.remaining[x], 1);
    }
}

// output assembly
__global__ void k_cl_flags(ClusterState S, int* is_solo, int* is_seed) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.n) return;
    is_solo[v] = (S.state[v] == 1) ? 1 : 0;
    is_seed[v] = S.seed[v];
}

// Clusters in one list: solos get key = index (top bit clear), picks key = ~pickkey (top bit
// set): an ascending sort lists solos by index, then picks by (remaining, index) descending.
__global__ void k_cl_list(const int* is_solo, const long long* spos, const int* is_seed, const long long* kpos,
                          long long nsolo, const unsigned long long* pickkey, int n, unsigned long long* sortkey, int* val) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    if (is_solo[v]) { sortkey[spos[v]] = static_cast<unsigned long long>(v); val[spos[v]] = v; }
    if (is_seed[v]) { sortkey[nsolo + kpos[v]] = ~pickkey[v]; val[nsolo + kpos[v]] = v; }
}

__global__ void k_cl_gidkey(const int* gid, const int* val, long long n, unsigned long long* key) {
    const long long c = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (c < n) key[c] = static_cast<unsigned long long>(gid[val[c]]);
}

__global__ void k_cl_sizes(ClusterState S, const int* order, long long nclu, int* sizes) {
    const long long c = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (c < nclu) sizes[c] = S.seed[order[c]] ? S.csize[order[c]] : 1;
}

__global__ void k_cl_write(ClusterState S, const int* order, long long nclu, const long long* coff,
                           const int32_t* members /* optional 1-based ids */, int32_t* out) {
    const long long c = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (c >= nclu) return;
    const int v = order[c];
    const long long o = coff[c];
    if (!S.seed[v]) { out[o] = members ? members[v] : v + 1; return; }
    const long long a = S.off[v];
    for (int k = 0; k < S.csize[v]; ++k) {
        const int w = S.memb[a + k];
        out[o + k] = members ? members[w] : w + 1;
    }
}

// ---------------------------------------------------------------------------
// device steps (umi_common.hpp); cluster_dev (umi_host.cpp) runs them

// one wavefront per node in the dense rounds, one thread per node otherwise
static dim3 per_node(const ClusterState& S) { return dim3(nblk(S.n, 256)); }
static dim3 per_node_w(const ClusterState& S) { return dim3(nblk(S.n, 4)); }
static const dim3 CL_B(256);

void gid_keys(const int* gid, const int* val, long long n, unsigned long long* key, hipStream_t s) {
    hipLaunchKernelGGL(k_cl_gidkey, dim3(nblk(n, 256)), CL_B, 0, s, gid, val, n, key);
}

// The state of a clustering and k_cl_init; herr: the four error indices it found (INT_MAX: none).
int cluster_begin(const DevAdj& adj, int n, bool check_sym, ClusterState* S, int herr[4], hipStream_t s) {
    const std::string p = UMI_WS[WS_CL];
    S->off = adj.off; S->nbr = adj.nbr; S->n = n;
    const size_t nn = static_cast<size_t>(n) + 1;
    SL_TRY(scratch(p + ".remaining", nn, &S->remaining));
    SL_TRY(scratch(p + ".state", nn, &S->state));
    SL_TRY(scratch(p + ".mark", nn, &S->mark));
    SL_TRY(scratch(p + ".key", nn, &S->key));
    SL_TRY(scratch(p + ".m1", nn, &S->m1));
    SL_TRY(scratch(p + ".seed", nn, &S->seed));
    SL_TRY(scratch(p + ".pickkey", nn, &S->pickkey));
    SL_TRY(scratch(p + ".memb", static_cast<size_t>(adj.nnz) + 1, &S->memb));
    SL_TRY(scratch(p + ".csize", nn, &S->csize));
    SL_TRY(scratch(p + ".err", 4, &S->err));
    SL_TRY(scratch(p + ".live", 1, &S->live));
    const int big = std::numeric_limits<int>::max();
    const int init[4] = {big, big, big, big};
    SL_HIP(hipMemcpyAsync(S->err, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_cl_init, per_node(*S), CL_B, 0, s, *S, check_sym ? 1 : 0);
    SL_HIP(hipMemcpyAsync(herr, S->err, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

// Scratch of the candidate-set rounds (dense graphs); control: with the control block, set to start them.
int cluster_candidates_begin(const ClusterState& S, bool control, ClusterTop* T, hipStream_t s) {
    const std::string p = UMI_WS[WS_CL];
    const size_t nn = static_cast<size_t>(S.n) + 1;
    SL_TRY(scratch(p + ".maxrem", 1, &T->maxrem));
    SL_TRY(scratch(p + ".counts", 4, &T->counts));
    SL_TRY(scratch(p + ".hop1", nn, &T->hop1));
    T->cap = std::max(1024, S.n / 8);
    SL_TRY(scratch(p + ".cand", static_cast<size_t>(T->cap), &T->cand));
    SL_HIP(hipMemsetAsync(T->counts, 0, 4 * sizeof(int), s));
    if (!control) return 0;
    SL_TRY(scratch(p + ".marked", nn, &T->marked));
    SL_TRY(scratch(p + ".ctl", CTL_N, &T->ctl));
    static const int hctl[CTL_N] = {CL_TOP, 0, 0, 0, 0, 0, 0, 0};
    SL_HIP(hipMemcpyAsync(T->ctl, hctl, sizeof hctl, hipMemcpyHostToDevice, s));
    SL_HIP(hipMemsetAsync(S.live, 0, sizeof(int), s));
    SL_HIP(hipMemsetAsync(T->maxrem, 0, sizeof(int), s));
    return 0;
}

// this round's keys; *live: how many nodes are left
int cluster_count_live(const ClusterState& S, int* live, hipStream_t s) {
    SL_HIP(hipMemsetAsync(S.live, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_cl_keys, per_node(S), CL_B, 0, s, S);
    *live = 0;
    SL_HIP(hipMemcpyAsync(live, S.live, sizeof *live, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

// CL_GROUP candidate-set rounds under the device's control (k_cl_control)
void rounds_candidates(const ClusterState& S, const ClusterTop& T, int* round, hipStream_t s) {
    for (int q = 0; q < CL_GROUP; ++q, ++*round) {
        hipLaunchKernelGGL(k_cl_keys_top, dim3(nblk(S.n, 1024)), dim3(1024), 0, s, S, T);
        hipLaunchKernelGGL(k_cl_control, dim3(1), dim3(1), 0, s, S, T);
        hipLaunchKernelGGL(k_cl_collect, per_node(S), CL_B, 0, s, S, T, 0);
        hipLaunchKernelGGL(k_cl_mark_top, dim3(1024), CL_B, 0, s, S, T);
        hipLaunchKernelGGL(k_cl_pick_top, dim3(1024), CL_B, 0, s, S, T, *round);
        hipLaunchKernelGGL(k_cl_commit_list, dim3(64), CL_B, 0, s, S, T);
        hipLaunchKernelGGL(k_cl_decrement_list, dim3(1024), CL_B, 0, s, S, T);
    }
}

// one round over every list, a wavefront per node (the keys are this round's already)
void round_dense(const ClusterState& S, int round, hipStream_t s) {
    hipLaunchKernelGGL(k_cl_m1_w, per_node_w(S), CL_B, 0, s, S);
    hipLaunchKernelGGL(k_cl_pick_w, per_node_w(S), CL_B, 0, s, S, round);
    hipLaunchKernelGGL(k_cl_commit, per_node(S), CL_B, 0, s, S, round);
    hipLaunchKernelGGL(k_cl_decrement_w, per_node_w(S), CL_B, 0, s, S, round);
}

// the same, a thread per node
void round_sparse(const ClusterState& S, int round, hipStream_t s) {
    hipLaunchKernelGGL(k_cl_m1, per_node(S), CL_B, 0, s, S);
    hipLaunchKernelGGL(k_cl_pick, per_node(S), CL_B, 0, s, S, round);
    hipLaunchKernelGGL(k_cl_commit, per_node(S), CL_B, 0, s, S, round);
    hipLaunchKernelGGL(k_cl_decrement, per_node(S), CL_B, 0, s, S, round);
}

// Output order -- solos by index, then picks by key descending, pre-group by pre-group -- and the clusters written in it.
int clusters_write(const ClusterState& S, const int32_t* d_members, const int* d_gid, int ngroups, ClusterResult* res, hipStream_t s) {
    const std::string p = UMI_WS[WS_CL];
    const int n = S.n;
    const size_t nn = static_cast<size_t>(n) + 1;
    const dim3 g = per_node(S), b = CL_B;
    int *d_issolo, *d_isseed, *d_order, *d_val, *d_val2, *d_sizes;
    long long *d_spos, *d_kpos;
    unsigned long long *d_sk, *d_sk2;
    SL_TRY(scratch(p + ".issolo", nn, &d_issolo));
    SL_TRY(scratch(p + ".isseed", nn, &d_isseed));
    SL_TRY(scratch(p + ".spos", nn, &d_spos));
    SL_TRY(scratch(p + ".kpos", nn, &d_kpos));
    SL_TRY(scratch(p + ".order", nn, &d_order));
    SL_TRY(scratch(p + ".val", nn, &d_val));
    SL_TRY(scratch(p + ".val2", nn, &d_val2));
    SL_TRY(scratch(p + ".sk", nn, &d_sk));
    SL_TRY(scratch(p + ".sk2", nn, &d_sk2));
    SL_TRY(scratch(p + ".sizes", nn, &d_sizes));
    hipLaunchKernelGGL(k_cl_flags, g, b, 0, s, S, d_issolo, d_isseed);
    SL_HIP(hipMemsetAsync(d_issolo + n, 0, sizeof(int), s));
    SL_HIP(hipMemsetAsync(d_isseed + n, 0, sizeof(int), s));
    SL_TRY(exclusive_scan(p + ".scantmp", d_issolo, d_spos, nn, s));
    SL_TRY(exclusive_scan(p + ".scantmp", d_isseed, d_kpos, nn, s));
    long long nsolo = 0, nseed = 0;
    SL_HIP(hipMemcpyAsync(&nsolo, d_spos + n, sizeof nsolo, hipMemcpyDeviceToHost, s));
    SL_HIP(hipMemcpyAsync(&nseed, d_kpos + n, sizeof nseed, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    const long long nclu = nsolo + nseed;
    if (nclu) {
        hipLaunchKernelGGL(k_cl_list, g, b, 0, s, d_issolo, d_spos, d_isseed, d_kpos, nsolo, S.pickkey, n, d_sk, d_val);
        SL_TRY(radix_sort_pairs(p + ".sorttmp", d_sk, d_sk2, d_val, d_val2, static_cast<size_t>(nclu), 64, s));
        if (d_gid && ngroups > 1) {  // stable: keeps the in-group order, groups in input order
            gid_keys(d_gid, d_val2, nclu, d_sk, s);
            SL_TRY(radix_sort_pairs(p + ".sorttmp", d_sk, d_sk2, d_val2, d_val, static_cast<size_t>(nclu),
                                    ceil_log2(static_cast<unsigned long long>(ngroups) + 1), s));
            SL_HIP(hipMemcpyAsync(d_order, d_val, sizeof(int) * static_cast<size_t>(nclu), hipMemcpyDeviceToDevice, s));
        } else {
            SL_HIP(hipMemcpyAsync(d_order, d_val2, sizeof(int) * static_cast<size_t>(nclu), hipMemcpyDeviceToDevice, s));
        }
    }
    long long* d_coff;
    int32_t* d_out;
    SL_TRY(scratch(p + ".coff", static_cast<size_t>(nclu) + 2, &d_coff));
    SL_TRY(scratch(p + ".out", nn, &d_out));
    if (nclu) {
        hipLaunchKernelGGL(k_cl_sizes, dim3(nblk(nclu, 256)), b, 0, s, S, d_order, nclu, d_sizes);
        SL_HIP(hipMemsetAsync(d_sizes + nclu, 0, sizeof(int), s));
        SL_TRY(exclusive_scan(p + ".scantmp", d_sizes, d_coff, static_cast<size_t>(nclu) + 1, s));
        hipLaunchKernelGGL(k_cl_write, dim3(nblk(nclu, 256)), b, 0, s, S, d_order, nclu, d_coff, d_members, d_out);
        SL_HIP(hipGetLastError());
        SL_HIP(hipMemcpyAsync(&res->total, d_coff + nclu, sizeof(long long), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
    } else {
        static const long long zero = 0;
        SL_HIP(hipMemcpyAsync(d_coff, &zero, sizeof zero, hipMemcpyHostToDevice, s));
        res->total = 0;
    }
    res->nclu = nclu;
    res->d_coff = d_coff;
    res->d_out = d_out;
    return 0;
}

}  // namespace sarlacc
