// umi_host.cpp -- host side of the UMI stage: everything that decides.  The kernels and the device steps that enqueue
// them are in umi_search.hip (encoding, tile search, split-key search), umi.hip (adjacency, dense distances) and
// umi_cluster.hip (greedy clustering); the plan structs and the steps' declarations in umi_common.hpp.
// Replaces compute_lev_masked (the reference's src/compute_lev_masked.cpp:13-64), sorted_trie's search
// (src/sorted_trie.cpp:107-278), cluster_umis (src/cluster_umis.cpp:7-112) and the per pre-group driver umi_group
// (src/umi_group.cpp:14-116).  Design: DESIGN.md "UMI stage".
//
// A search is plan_search (what runs: SearchPlan) -> build (split orders, tile list) -> an optional sampled pass that
// sizes the pair buffer -> the search, once more when the buffer overflowed (pair_edges).  A clustering is cluster_dev:
// the rounds of one of three kinds, under the control block's or the live count's read-back.
#include "umi_common.hpp"

#include "../../include/sarlacc_amd.h"

namespace sarlacc {

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// number of pairs the last sarlacc_dev_umi_pairs_shard of this thread left in the workspace buffer "u1.edges" (-1: none);
// every pair_edges call on "u1" reuses that buffer, so it is reset before one
static thread_local long long g_shard_pairs = -1;

// ---------------------------------------------------------------------------
// encoding

// how an entry path names its strings in the two errors of the encode
struct EncodeTexts { const char* what; const char* bad_char_note; };
constexpr EncodeTexts UMI_TEXTS{"UMI", " (the reference silently drops such strings)"};
// characters outside ACGTN behave as ordinary distinct letters in the reference
// (src/compute_lev_masked.cpp:51); only ACGTN is supported here
constexpr EncodeTexts LEV_TEXTS{"sequence", ""};

// Encode in input order, at as many words as the longest string needs: 1 up to 32 bases, 4 up to 128 (tiles staged in
// LDS), beyond as many as the longest string takes.
static int encode(const std::string& p, const EncodeIn& in, const EncodeTexts& t, Encoded* e, int* words, hipStream_t s) {
    const int none = std::numeric_limits<int>::max();
    SL_TRY(encode_at(p, in, 1, 0, e, s));
    *words = 1;
    if (e->too_long != none) {
        // some string has more than 32 bases: the whole call runs on multi-word codes
        const int maxlen = e->maxlen;
        if (maxlen > UMI_XL_MAX) return fail("sarlacc_amd: %s longer than %d bases is not supported", t.what, UMI_XL_MAX);
        *words = maxlen <= UMI_LONG_MAX ? UMI_LONG_WORDS : (maxlen + 31) / 32;
        SL_TRY(encode_at(p, in, *words, maxlen, e, s));
        e->maxlen = maxlen;
    }
    if (e->bad_char != none) return fail("sarlacc_amd: %s contains a character outside ACGTN%s", t.what, t.bad_char_note);
    return 0;
}

// Encode one set of UMIs (optionally the members of a pre-group) and order it like the trie.
static int encode_and_rank(const std::string& p, const uint8_t* d_chars, const int64_t* d_off, const int32_t* d_members,
                           const int* d_gid, int ngroups, int n, SortedUmis* out, hipStream_t s, const uint8_t* d_skip = nullptr,
                           int nskip = 0, int max_group = 0) {
    out->nskip = d_skip ? nskip : 0;
    out->max_group = max_group > 0 ? max_group : n;
    Encoded e{};
    int words;
    SL_TRY(encode(p, EncodeIn{d_chars, d_off, d_members, d_skip, n}, UMI_TEXTS, &e, &words, s));
    return rank_umis(p, e, words, d_gid, ngroups, n, out, s);
}

// ---------------------------------------------------------------------------
// the neighbour search

constexpr int SK_MIN_N = 32768;          // below this (or with pre-groups averaging under half of it) the all-tile-pairs search is quick enough
constexpr int FILTER_MAX_LIMIT = 5;      // the tile filter's prefix distances: k_tile_pairs<0..5>
constexpr int FILTER_MIN_TILES = 16;     // worth it from a few dozen tiles on
constexpr long long FILTER_MAX_TILE_PAIRS = 1ll << 31;
constexpr unsigned SAMPLE_STRIDE = 32;   // the sampled pass: every 32nd listed tile pair and work item of the scans ...
constexpr long long SAMPLE_MIN = 2048;   // ... when there are this many of either

// The lengths present decide the scans: one class per length 8..15 and one for 16 and longer.
static int sk_plan(const std::string& p, const SortedUmis& S, int limit, SkPlan* plan, hipStream_t s) {
    unsigned int hist[34];
    SL_TRY(length_hist(p, S, hist, s));
    plan->classes.clear();
    for (int L = SK_MIN_LEN; L <= 2 * SK_MAX_KEY; ++L) {
        long long rows = hist[L];
        if (L == 2 * SK_MAX_KEY) for (int M = L + 1; M <= 32; ++M) rows += hist[M];
        if (!rows) continue;
        const int h = std::min(L / 2, SK_MAX_KEY), len_hi = L == 2 * SK_MAX_KEY ? 32 : L;
        // two candidate columns per lane for the rows no string of 16 and more bases can be a neighbour of (the lengths of
        // neighbours differ by `limit` at most; such columns are simply not valid there)
        const bool two = len_hi + limit < 16 && !option(OPT_UMI_SCAN_SINGLE);
        plan->classes.push_back(SkClass{L, len_hi, h, std::min(L - h, SK_MAX_KEY), two});
    }
    plan->k1 = limit >= 2 ? 1 : 0;   // limit 1: both keys have to match exactly; 2: the suffix key; 3: one edit in either
    plan->k2 = limit - 1 - plan->k1;
    long long shorter = 0;
    for (int L = 0; L < SK_MIN_LEN; ++L) shorter += hist[L];
    plan->nspecial = shorter + hist[33];   // an upper bound (short strings with an N count twice)
    return 0;
}

// the smallest band of `bands` that holds the limit; `beyond` past the last
static int band_of(int limit, std::initializer_list<int> bands, int beyond) {
    for (int k : bands) if (limit <= k) return k;
    return beyond;
}

// What one search runs.  (tile_hi < 0: every row tile.)  The one device read is the length histogram of sk_plan.
static int plan_search(const std::string& p, const SortedUmis& S, int limit, int tile_lo, int tile_hi, SearchPlan* P, hipStream_t s) {
    const int n = S.n;
    P->limit = limit;
    P->words = S.words;
    P->xl = S.words > UMI_LONG_WORDS;
    P->nt = static_cast<int>(nblk(n, TILE));
    if (tile_hi < 0) { tile_lo = 0; tile_hi = P->nt; }
    P->tile_lo = std::max(0, std::min(tile_lo, P->nt));
    P->tile_hi = std::max(P->tile_lo, std::min(tile_hi, P->nt));
    P->row_lo = static_cast<uint32_t>(std::min<long long>(static_cast<long long>(P->tile_lo) * TILE, n));
    P->row_hi = static_cast<uint32_t>(std::min<long long>(static_cast<long long>(P->tile_hi) * TILE, n));
    // Thresholds 1 to 3 on a large set: candidates from the split keys (see k_sk_scan); the tile kernel then only
    // looks at the pairs with a "special" member, if there are any.
    // (the largest pre-group decides, not the average: a set with one large pre-group among thousands of small ones has the
    // quadratic tile search to lose; the reads that sit alone in their pre-group are encoded as empty strings, take no part
    // in any comparison and are not "special")
    const int min_n = option(OPT_UMI_SPLIT_MIN) > 0 ? option(OPT_UMI_SPLIT_MIN) : SK_MIN_N;
    P->split = S.words == 1 && limit >= 1 && limit <= 3 && n >= min_n && !option(OPT_UMI_TILE_SEARCH) && S.max_group >= min_n / 2;
    if (P->split) {
        SL_TRY(sk_plan(p, S, limit, &P->sk, s));
        P->sk.nspecial = std::max<long long>(0, P->sk.nspecial - S.nskip);
        P->split = !P->sk.classes.empty() && 4 * P->sk.nspecial <= n - S.nskip;
    }
    P->special_lreq = P->split ? SK_MIN_LEN : -1;
    P->tiles = !P->split || P->sk.nspecial > 0;
    // tile pairs that can hold neighbours (see k_tile_pairs)
    const long long ntp = static_cast<long long>(P->tile_hi - P->tile_lo) * P->nt;
    P->filter = P->tiles && S.words == 1 && limit >= 0 && limit <= FILTER_MAX_LIMIT && P->nt >= FILTER_MIN_TILES && ntp <= FILTER_MAX_TILE_PAIRS;
    P->L = P->filter ? limit : 0;
    if (!P->tiles || limit < 0) P->K = PAIRS_K_NONE;   // (nothing can match a negative limit: no search kernel at all)
    else if (S.words > 1) P->K = band_of(limit, {0, 1, 2, 3, 5, 8, 16}, PAIRS_K_FULL);
    else P->K = band_of(std::min(limit, UMI_MAXLEN), {0, 1, 2, 3, 4, 5, 8, 16}, UMI_MAXLEN);
    // a sample of the tile kernel's work needs the list
    const bool sample = limit >= 0 && (!P->tiles || P->filter);
    P->sample_tiles = sample && P->filter;
    P->sample_items = sample && P->split;
    return 0;
}

// Every search kernel of one pass over the set; `stride` > 1: a sample (every stride-th listed tile pair / work item).
static int search_pass(const SortedUmis& S, const SearchPlan& P, const SplitOrders& O, const TileList& T, unsigned stride,
                       const PairBuffer& b, hipStream_t s) {
    if (P.split && P.row_hi > P.row_lo) {
        long long items;
        int two_columns;
        split_scans(O, P, stride, b, &items, &two_columns, s);
        ctx().counts["umi_split_items"] = static_cast<double>(items);
        ctx().counts["umi_scan_two_columns"] = two_columns;   // launches of k_sk_scan_pk
    }
    if (P.tiles) SL_TRY(pair_search(S, P, T, stride, b, s));
    return 0;
}

// All neighbour pairs within `limit` among the rows of the tiles tile_lo..tile_hi (tile_hi < 0: all), as
// (rank_i << 32 | rank_j), rank_i < rank_j, in the workspace buffer "<p>.edges".
static int pair_edges(const std::string& p, const SortedUmis& S, int limit, int tile_lo, int tile_hi,
                      unsigned long long** d_edges_out, unsigned long long* m_out, hipStream_t s) {
    Context& c = ctx();
    const int n = S.n;
    PairBuffer b{nullptr, nullptr, std::max<unsigned long long>(1u << 20, 32ull * n)};
    SL_TRY(scratch(p + ".ecount", 1, &b.count));
    if (n > static_cast<long long>(65535) * TILE) return fail("sarlacc_amd: more than %d UMIs in one call", 65535 * TILE);
    auto edges_buffer = [&]() {
        void* pe;
        SL_TRY(c.buffer((p + ".edges").c_str(), b.cap * sizeof(unsigned long long), &pe));
        b.edges = static_cast<unsigned long long*>(pe);
        return 0;
    };
    SL_TRY(edges_buffer());   // make sure a buffer exists even when nothing is launched

    SearchPlan P;
    SL_TRY(plan_search(p, S, limit, tile_lo, tile_hi, &P, s));
    c.counts["umi_pairs_words"] = P.words;
    c.counts["umi_pairs_k"] = P.K;
    c.counts["umi_split_search"] = P.split ? 1 : 0;
    c.counts["umi_split_classes"] = P.split ? static_cast<double>(P.sk.classes.size()) : 0;
    c.counts["umi_split_special"] = P.split ? static_cast<double>(P.sk.nspecial) : 0;
    c.counts["umi_split_items"] = 0;

    SplitOrders O;
    TileList T;
    if (P.split) SL_TRY(split_orders(p, S, P.sk, &O, s));
    if (P.filter) SL_TRY(tile_filter(p, S, P, &T, s));
    // what the tile filter kept: upper-triangle tile pairs of this launch, and how many of them are searched (0: no list)
    const long long ntp = static_cast<long long>(P.tile_hi - P.tile_lo) * P.nt;
    const long long below_diagonal = static_cast<long long>(P.tile_lo + P.tile_hi - 1) * (P.tile_hi - P.tile_lo) / 2;   // sum of the row tiles' indices
    c.counts["umi_tile_pairs_total"] = static_cast<double>(ntp - below_diagonal);
    c.counts["umi_tile_pairs_listed"] = static_cast<double>(T.n);

    // Capacity of the pair buffer: 32 per element covers thresholds 1 and 2; dense neighbourhoods (threshold 3 on 12-base
    // UMIs: hundreds of neighbours each) would overflow it and cost a second full search, so the density is first
    // estimated from a sample: every 32nd listed tile pair (k_tile_pairs appends them in no particular order) and
    // every 32nd work item of the split-key scans.
    long long all_items = 0;
    for (const SkScan& q : O.fwd) all_items += q.nitems;
    for (const SkScan& q : O.rev) all_items += q.nitems;
    if ((P.sample_tiles && T.n >= SAMPLE_MIN) || (P.sample_items && all_items >= SAMPLE_MIN)) {
        SL_HIP(hipMemsetAsync(b.count, 0, sizeof(unsigned long long), s));
        SL_TRY(search_pass(S, P, O, T, SAMPLE_STRIDE, b, s));
        SL_HIP(hipGetLastError());
        unsigned long long ms = 0;
        SL_HIP(hipMemcpyAsync(&ms, b.count, sizeof ms, hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        const double est = static_cast<double>(ms) * SAMPLE_STRIDE;
        b.cap = std::max<unsigned long long>(b.cap, static_cast<unsigned long long>(est * 1.25) + (1u << 20));
        c.counts["umi_pairs_estimated"] = est;
    }
    unsigned long long m = 0;
    for (int attempt = 0; attempt < 2 && limit >= 0; ++attempt) {
        SL_TRY(edges_buffer());
        SL_HIP(hipMemsetAsync(b.count, 0, sizeof(unsigned long long), s));
        SL_HIP(hipEventRecord(c.ev_start, s));
        c.stage_reset("umi_pairs");
        SL_TRY(c.stage_begin("umi_pairs", s));
        SL_TRY(search_pass(S, P, O, T, 1u, b, s));
        SL_HIP(hipGetLastError());
        SL_HIP(hipEventRecord(c.ev_stop, s));
        SL_TRY(c.stage_end("umi_pairs", s));
        c.timed = true;
        SL_HIP(hipMemcpyAsync(&m, b.count, sizeof m, hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        c.counts["umi_pair_attempts"] = attempt + 1;
        if (m <= b.cap) break;
        b.cap = m;  // the kernels kept counting: second attempt has the exact size
    }
    *d_edges_out = b.edges;
    *m_out = m;
    return 0;
}

// Directed, sorted adjacency keys (self links included) from undirected rank pairs.
static int keys_from_edges(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single,
                           const unsigned long long* d_edges, unsigned long long m, DirectedKeys* out, hipStream_t s) {
    SelfLinks self;
    SL_TRY(self_links(p, S, limit, d_single, &self, s));
    const long long nk = 2 * static_cast<long long>(m) + self.n;
    // The neighbour lists are explicit (as the reference's are, src/umi_group.cpp:59-103): 20 bytes per link while they are
    // sorted.  Measured up to 2.8e9 links (7e5 12-base UMIs at threshold 4: 4 000 neighbours each); beyond 2^32 the
    // call stops here instead of running out of memory half way.
    if (nk > 0xFFFFFFFFll)
        return fail("sarlacc_amd: %lld neighbour links in one call (at most 4294967295): the threshold joins most of the set -- "
                    "lower it or split the reads into pre-groups", nk);
    return directed_keys(p, S, d_edges, m, self, out, s);
}

// All neighbour pairs within `limit`, as sorted directed keys (self links included).
static int neighbour_keys(const std::string& p, const SortedUmis& S, int limit, const uint8_t* d_single, DirectedKeys* out, hipStream_t s) {
    if (limit < 0) limit = -1;  // nothing can match a negative limit
    unsigned long long* d_edges;
    unsigned long long m;
    const double t0 = now();
    SL_TRY(pair_edges(p, S, limit, 0, -1, &d_edges, &m, s));
    ctx().counts["umi_pair_search_s"] = now() - t0;
    return keys_from_edges(p, S, limit, d_single, d_edges, m, out, s);
}

// Neighbour lists for one group: UMI1 only, or UMI1 n UMI2 listed in UMI2's order
// (src/umi_group.cpp:59-103).
static int group_adjacency(const uint8_t* d_c1, const int64_t* d_o1, const uint8_t* d_c2, const int64_t* d_o2,
                           const int32_t* d_members, const int* d_gid, const uint8_t* d_single, int ngroups, int n,
                           int limit1, int limit2, DevAdj* adj, hipStream_t s, int nsingle = 0, int max_group = 0) {
    const std::string u1 = UMI_WS[WS_U1], u2 = UMI_WS[WS_U2];
    SortedUmis S1;
    DirectedKeys K1;
    auto synced_now = [&] { (void)hipStreamSynchronize(s); return now(); };
    const double t0 = synced_now();
    SL_TRY(encode_and_rank(u1, d_c1, d_o1, d_members, d_gid, ngroups, n, &S1, s, d_single, nsingle, max_group));
    const double t1 = synced_now();
    g_shard_pairs = -1;
    SL_TRY(neighbour_keys(u1, S1, limit1, d_single, &K1, s));
    const double t2 = synced_now();
    ctx().counts["umi_encode_sort_s"] = t1 - t0;
    ctx().counts["umi_search_and_key_sort_s"] = t2 - t1;
    if (!d_c2) return adjacency_from_keys(K1.keys, K1.nk, S1.perm, n, adj, s);

    unsigned long long* d_s1;
    SL_TRY(link_set(u1, K1, S1.perm, &d_s1, s));
    SortedUmis S2;
    DirectedKeys K2, kept;
    SL_TRY(encode_and_rank(u2, d_c2, d_o2, d_members, d_gid, ngroups, n, &S2, s, d_single, nsingle, max_group));
    SL_TRY(neighbour_keys(u2, S2, limit2, d_single, &K2, s));
    SL_TRY(links_in_set(u2, K2, S2.perm, d_s1, K1.nk, &kept, s));
    return adjacency_from_keys(kept.keys, kept.nk, S2.perm, n, adj, s);
}

// ---------------------------------------------------------------------------
// clustering

// Greedy clustering of a device CSR graph.  `check_sym`: symmetric lists are the documented
// precondition of this implementation (the reference's results on asymmetric input
// are an accident of its update order; umi_group always produces symmetric lists).
static int cluster_dev(const DevAdj& adj, int n, const int32_t* d_members, const int* d_gid, int ngroups, bool check_sym,
                       ClusterResult* res, hipStream_t s) {
    ClusterState S{};
    int herr[4];
    // one wavefront per node from 24 links per node on average (one thread per node below that)
    const bool dense = adj.nnz >= 24LL * n;
    ctx().counts["umi_links"] = static_cast<double>(adj.nnz);
    ctx().counts["umi_cluster_candidate_rounds"] = 0;
    ctx().counts["umi_cluster_full_rounds"] = 0;
    ctx().counts["umi_cluster_widened"] = 0;
    ctx().counts["umi_cluster_narrowed"] = 0;
    SL_TRY(cluster_begin(adj, n, check_sym, &S, herr, s));
    const int big = std::numeric_limits<int>::max();
    // first error in index order, as the reference's loop would meet it (src/cluster_umis.cpp:21-40)
    if (herr[0] != big || herr[1] != big) {
        if (herr[0] < herr[1]) return fail("zero length read group");
        return fail("single-read groups should contain only the read itself");
    }
    // (a read named twice in a list: the reference skips the second mention, k_cl_pick would store both)
    if (herr[3] != big && herr[3] <= herr[2]) return fail("sarlacc_amd: list %d names a read twice", herr[3] + 1);
    if (herr[2] != big)
        return fail("sarlacc_amd: neighbour lists must be symmetric and contain the read itself (list %d is not)", herr[2] + 1);

    const bool top_rounds = dense && !option(OPT_UMI_FULL_ROUNDS);
    ClusterTop T{};
    if (dense) SL_TRY(cluster_candidates_begin(S, top_rounds, &T, s));
    long long top_rounds_run = 0, full_rounds_run = 0;
    int rounds_total = 0, widened = 0, narrowed = 0;
    if (top_rounds) {
        // Candidate-set rounds under the device's control (k_cl_control): CL_GROUP rounds per read-back.  A round whose list
        // was cut off parks the control block (CL_WANTS_FULL; the rounds still queued behind it do nothing) and the host
        // runs that round over every list, as before.
        int hctl[CTL_N];
        int round = 0;
        for (;;) {
            rounds_candidates(S, T, &round, s);
            SL_HIP(hipGetLastError());
            SL_HIP(hipMemcpyAsync(hctl, T.ctl, sizeof hctl, hipMemcpyDeviceToHost, s));
            SL_HIP(hipStreamSynchronize(s));
            if (hctl[CTL_MODE] == CL_DONE) break;
            if (hctl[CTL_MODE] == CL_WANTS_FULL) {   // (the keys are those of the round that asked: nothing changed since)
                round_dense(S, round, s);
                ++round; ++full_rounds_run;
                const int back[3] = {CL_TOP, hctl[CTL_DELTA], 0};
                SL_HIP(hipMemcpyAsync(T.ctl, back, sizeof back, hipMemcpyHostToDevice, s));
                SL_HIP(hipStreamSynchronize(s));   // (`back` is on this frame)
            }
            if (hctl[CTL_ROUNDS] + full_rounds_run > 4LL * n + 16) return fail("sarlacc_amd: clustering did not converge");
        }
        top_rounds_run = hctl[CTL_ROUNDS];
        widened = hctl[CTL_WIDENED]; narrowed = hctl[CTL_NARROWED];
        rounds_total = static_cast<int>(top_rounds_run + full_rounds_run);
    } else {
        for (int round = 0;; ++round) {
            int live;
            SL_TRY(cluster_count_live(S, &live, s));
            if (live == 0) break;
            if (dense) round_dense(S, round, s);
            else round_sparse(S, round, s);
            SL_HIP(hipGetLastError());
            if (round > 4 * n + 16) return fail("sarlacc_amd: clustering did not converge");
            ++full_rounds_run;
            rounds_total = round + 1;
        }
    }
    ctx().counts["umi_cluster_rounds"] = rounds_total;
    ctx().counts["umi_cluster_candidate_rounds"] = static_cast<double>(top_rounds_run);
    ctx().counts["umi_cluster_full_rounds"] = static_cast<double>(full_rounds_run);
    // rounds after which k_cl_control doubled / halved the candidate window
    ctx().counts["umi_cluster_widened"] = widened;
    ctx().counts["umi_cluster_narrowed"] = narrowed;
    return clusters_write(S, d_members, d_gid, ngroups, res, s);
}

// the clusters to the caller's arrays
static int clusters_out(const ClusterResult& res, int64_t* nclusters, int64_t* clu_off, int32_t* clu) {
    std::vector<long long> co(static_cast<size_t>(res.nclu) + 1);
    SL_HIP(hipMemcpy(co.data(), res.d_coff, sizeof(long long) * co.size(), hipMemcpyDeviceToHost));
    if (res.total) SL_HIP(hipMemcpy(clu, res.d_out, sizeof(int32_t) * static_cast<size_t>(res.total), hipMemcpyDeviceToHost));
    for (long long c = 0; c <= res.nclu; ++c) clu_off[c] = co[c];
    *nclusters = res.nclu;
    return 0;
}

// ---------------------------------------------------------------------------
// what the entry points share

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

// The pairs of one shard's row tiles, left in the workspace buffer "u1.edges".
static int shard_search(const char* umi, const int64_t* off, int64_t n, int limit, int shard_index, int shard_count,
                        unsigned long long** d_edges, unsigned long long* m, hipStream_t s) {
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_PS, umi, off, n, &d_c, &d_o, s));
    SortedUmis S;
    SL_TRY(encode_and_rank(UMI_WS[WS_U1], d_c, d_o, nullptr, nullptr, 1, static_cast<int>(n), &S, s));
    int lo, hi;
    shard_tiles(static_cast<int>(nblk(n, TILE)), shard_index, shard_count, &lo, &hi);
    g_shard_pairs = -1;
    return pair_edges(UMI_WS[WS_U1], S, limit, lo, hi, d_edges, m, s);
}

// What the two group_from_pairs entry points answer by themselves; *done: nothing is left to do.
static int pairs_prologue(int64_t n, int64_t npairs, bool null_buffer, int64_t* nclusters, int64_t* clu_off, int32_t* clu, bool* done) {
    *done = true;
    if (n < 0 || npairs < 0) return fail("sarlacc_amd: negative sizes");
    if (null_buffer) return fail("sarlacc_amd: null pair buffer");
    *nclusters = 0;
    clu_off[0] = 0;
    if (n == 0) return 0;
    if (n == 1) {  // a pre-group of one read passes through (src/umi_group.cpp:39-42)
        clu[0] = 1; clu_off[1] = 1; *nclusters = 1;
        return 0;
    }
    *done = false;
    return 0;
}

// clustering of ONE pre-group from its neighbour pairs, which are already on the device (validated there)
static int group_from_device_pairs(const char* umi, const int64_t* off, int64_t n, int limit, const unsigned long long* d_edges,
                                   int64_t npairs, int64_t* nclusters, int64_t* clu_off, int32_t* clu, hipStream_t s) {
    uint8_t* d_c; int64_t* d_o;
    SL_TRY(upload_strings(WS_PS, umi, off, n, &d_c, &d_o, s));
    SortedUmis S;
    SL_TRY(encode_and_rank(UMI_WS[WS_U1], d_c, d_o, nullptr, nullptr, 1, static_cast<int>(n), &S, s));
    int bad;
    SL_TRY(check_pairs(d_edges, npairs, n, &bad, s));
    if (bad) return fail("sarlacc_amd: malformed neighbour pair");
    const double t0 = now();
    DirectedKeys K;
    SL_TRY(keys_from_edges(UMI_WS[WS_U1], S, limit < 0 ? -1 : limit, nullptr, d_edges, static_cast<unsigned long long>(npairs), &K, s));
    DevAdj adj;
    SL_TRY(adjacency_from_keys(K.keys, K.nk, S.perm, static_cast<int>(n), &adj, s));
    SL_HIP(hipStreamSynchronize(s));
    const double t1 = now();
    ClusterResult res;
    SL_TRY(cluster_dev(adj, static_cast<int>(n), nullptr, nullptr, 1, false, &res, s));
    ctx().counts["umi_adjacency_s"] = t1 - t0;
    ctx().counts["umi_cluster_s"] = now() - t1;
    return clusters_out(res, nclusters, clu_off, clu);
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
    Encoded e{};
    int words;
    SL_TRY(encode(p, EncodeIn{d_c, d_o, nullptr, nullptr, static_cast<int>(n)}, LEV_TEXTS, &e, &words, s));
    double* d_out;
    SL_TRY(dense_distances(p, e.raw, static_cast<int>(n), words, &d_out, s));
    SL_HIP(hipMemcpy(out, d_out, sizeof(double) * static_cast<size_t>(n * (n - 1) / 2), hipMemcpyDeviceToHost));
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
    return clusters_out(res, nclusters, clu_off, clu);
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
        SL_TRY(clusters_out(res, nclusters, clu_off, clu));
        ctx().counts["umi_tables_in_s"] = t0 - t_in;    // strings and pre-group tables to the device
        ctx().counts["umi_clusters_out_s"] = now() - t2;
    }
    return 0;
}

int sarlacc_umi_pairs_shard(const char* umi, const int64_t* off, int64_t n, int limit, int shard_index,
                            int shard_count, uint64_t* pairs, int64_t cap, int64_t* npairs) {
    if (n < 0 || shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return fail("sarlacc_amd: bad shard request");
    *npairs = 0;
    if (n == 0 || limit < 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    unsigned long long* d_edges;
    unsigned long long m;
    SL_TRY(shard_search(umi, off, n, limit, shard_index, shard_count, &d_edges, &m, s));
    *npairs = static_cast<int64_t>(m);
    if (!pairs || cap < static_cast<int64_t>(m)) return 0;  // sizing call
    if (m) SL_HIP(hipMemcpy(pairs, d_edges, sizeof(uint64_t) * m, hipMemcpyDeviceToHost));
    return 0;
}

int sarlacc_umi_group_from_pairs(const char* umi, const int64_t* off, int64_t n, int limit, const uint64_t* pairs,
                                 int64_t npairs, int64_t* nclusters, int64_t* clu_off, int32_t* clu) {
    bool done;
    SL_TRY(pairs_prologue(n, npairs, false, nclusters, clu_off, clu, &done));
    if (done) return 0;
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
    unsigned long long* d_edges;
    unsigned long long m;
    SL_TRY(shard_search(umi, off, n, limit, shard_index, shard_count, &d_edges, &m, s));
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
    bool done;
    SL_TRY(pairs_prologue(n, npairs, npairs && !d_pairs, nclusters, clu_off, clu, &done));
    if (done) return 0;
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
