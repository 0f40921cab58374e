// sketch.hpp -- what sketch.hip and links_verify.hip (the kernels and the functions that launch them) and sketch_host.cpp
// (argument checks, scratch, the rocPRIM sorts and scans between the launches, results and errors, the C entry points) share.
#pragma once

#include "common.hpp"

namespace sarlacc {

constexpr uint64_t SK_EMPTY = ~0ull;      // an empty bucket of a sketch; a k-mer whose hash is this value counts as absent
constexpr int SK_MAX_BUCKETS = 256;       // 2 KB of LDS per wavefront

// ---- what the host sides of the sketch calls share (sketch_host.cpp, ref_map_host.cpp) ----
constexpr long long SK_LIMIT = 1LL << 31;

inline int count_ok(int64_t n, const char* what) {
    if (n < 0) return fail("sarlacc_amd: negative number of %s", what);
    if (n >= SK_LIMIT) return fail("sarlacc_amd: %lld %s: at most 2^31 - 1", static_cast<long long>(n), what);
    return 0;
}

// log2 of a power of two in 16 .. 256, -1 otherwise
inline int buckets_log2(int buckets) {
    for (int b = 4; b <= 8; ++b)
        if (buckets == 1 << b) return b;
    return -1;
}

// `body` as one segment of the stage timer `name`, which starts a new call
template <typename F>
int staged(const char* name, hipStream_t s, F&& body) {
    Context& c = ctx();
    c.stage_reset(name);
    SL_TRY(c.stage_begin(name, s));
    SL_TRY(body());
    return c.stage_end(name, s);
}

// The words a call's kernels report through (one scratch block, set up by sk_state_reset): every `bad_*` is an atomicMin
// over ~0, the counters are sums.
struct SkState {
    unsigned long long bad_off;       // lowest read whose offsets do not ascend inside the buffer
    unsigned long long bad_link;      // lowest link with an endpoint outside 0 .. n - 1
    unsigned long long n_pairs;       // distinct candidate pairs
    unsigned long long n_links, n_groups;
    unsigned int changed;             // a hook round moved a root
    unsigned long long n_kept;        // links that passed the alignment check
    unsigned long long n_second;      // pairs whose reverse orientation was computed
};

struct SketchArgs {
    const uint8_t* seq;
    const int64_t* off;
    long long n;
    int k, log2_buckets, canonical;
};

// a launch of the alignment check (rule 6a): w the bandwidth, 0 .. 127
struct VerifyArgs {
    const uint8_t* seq;
    const int64_t* off;
    long long n;
    const uint64_t* links;
    long long n_links;
    int w;
    long long max_diff_ppm;
    int both_strands;
};

// ---- sketch.hip ----
int sk_state_reset(SkState* d_state, hipStream_t s);
// sketch: n << log2_buckets words; nkmers: n
int launch_sketch(const SketchArgs& a, uint64_t* sketch, int32_t* nkmers, SkState* st, hipStream_t s);
// read[e] = e >> log2_buckets for the m = n << log2_buckets entries
int launch_sk_entry_reads(long long m, int log2_buckets, int32_t* read, hipStream_t s);
// Over the m entries sorted by (hash, read): count[p] (m + 1 entries, count[m] = 0) is the number of entries at distance
// 1 .. window behind p that hold the same hash; the fill pass writes, from begin[p] on (the m + 1 scanned counts),
// read[p] << bits | read[p + d].
int launch_sk_pairs_count(const uint64_t* hash, long long m, int window, int32_t* count, hipStream_t s);
int launch_sk_pairs_fill(const int32_t* read, long long m, const int64_t* begin, int bits, uint64_t* pair, hipStream_t s);
// Over the t pair keys in ascending order: flag[p] (t + 1 entries, flag[t] = 0) marks the head of a run of at least
// min_shared equal keys; the heads of all runs are counted into st->n_pairs.
int launch_sk_link_flags(const uint64_t* pair, long long t, int min_shared, int32_t* flag, SkState* st, hipStream_t s);
// links[before[p]] = a << 32 | b for the flagged p with before[p] < capacity; st->n_links = before[t]
int launch_sk_link_scatter(const uint64_t* pair, long long t, int bits, const int32_t* flag, const int64_t* before, uint64_t* links,
                           long long capacity, SkState* st, hipStream_t s);

int launch_cc_init(long long n, int32_t* parent, hipStream_t s);
// one round: every link whose two roots differ lowers the larger root to the smaller (atomicMin) and sets st->changed
int launch_cc_hook(const uint64_t* links, long long n_links, long long n, const int32_t* nkmers, int32_t* parent, SkState* st,
                   hipStream_t s);
// parent[v] = the root of v
int launch_cc_jump(long long n, int32_t* parent, hipStream_t s);
// head[v] (n + 1 entries, head[n] = 0): v is the root of a counted component
int launch_cc_heads(const int32_t* parent, const int32_t* nkmers, long long n, int32_t* head, hipStream_t s);
int launch_cc_labels(const int32_t* parent, const int32_t* nkmers, long long n, const int32_t* before, int32_t* label, SkState* st,
                     hipStream_t s);

// ---- links_verify.hip ----
// Per link (n_links > 0): dist (-1: the link fails), strand (may be null), flag[p] (n_links + 1 entries, flag[n_links] = 0)
// marks a link that passes; the lowest link with ends outside 0 <= a < b < n goes to st->bad_link, the lowest read with
// bad offsets to st->bad_off (such links fail), the pairs whose second strand was computed are counted into st->n_second.
int launch_links_verify(const VerifyArgs& a, int32_t* dist, uint8_t* strand, int32_t* flag, SkState* st, hipStream_t s);
// kept[before[p]] = links[p] for the flagged p (kept may be null); st->n_kept = before[n_links]
int launch_links_keep(const uint64_t* links, long long n_links, const int32_t* flag, const int64_t* before, uint64_t* kept, SkState* st,
                      hipStream_t s);

}  // namespace sarlacc
