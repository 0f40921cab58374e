// msa2_host.cpp -- the host side of the MSA stage above the spec v2 kernels (msa2.hip): the scoring domain, the split into
// spec v1 and spec v2 groups and the final gather (msa_run), the batch plan and its worker threads, the memory budget and
// the cut into pipelined batches, the row buffer that grows in place, the stage's work counters.
#include "msa2.hpp"

#include "../../include/sarlacc_amd.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <utility>

namespace sarlacc {

static int msa_spec() { return option(OPT_MSA_SPEC) == 1 ? 1 : 2; }

// ---- the stage's counters (sarlacc_stage_count): msa_run sets every one of them to 0, msa2_core adds a call's values, m2_host_time its seconds ----
constexpr int M2_ELSEWHERE = -1;     // filled by msa_pairwise.hip (or by nothing), set to 0 with the rest
constexpr int M2_EVERY_ROUTE = -2;   // filled by msa_pairwise.hip / msa_run, set to 0 on every route into the stage (spec v1 alone included)
struct M2Count { const char* name; int from; };   // from: M2C_* (the merge kernels' counters, m2_merge), M2H_*, or one of the two above
static const M2Count m2_counts[] = {
    {"msa_pairs", M2H_PAIRS}, {"msa_cells", M2H_CELLS},
    {"msa2_rows", M2C_ROWS}, {"msa2_rows_capped", M2C_ROWS_CAPPED}, {"msa2_entries_filtered", M2C_ENT_FILTERED},
    {"msa2_rows_filtered", M2C_ROWS_FILTERED}, {"msa2_entries_kept", M2C_ENT_KEPT}, {"msa2_joins", M2C_JOINS},
    {"msa2_joins_chain_in_hbm", M2C_JOINS_HBMQ}, {"msa2_gathers", M2C_GATHERS},
    {"msa2_groups_second_pass", M2H_SECOND_PASS}, {"msa2_batches", M2H_BATCHES},
    {"msa2_cycles_rows", M2C_CYC_ROWS}, {"msa2_cycles_chain", M2C_CYC_CHAIN}, {"msa2_cycles_walk", M2C_CYC_WALK},
    {"msa2_cycles_renumber", M2C_CYC_RENUMBER}, {"msa2_launches", M2C_T_START}, {"msa2_first_exit_s", M2C_T_FIRST_EXIT},
    {"msa2_last_exit_s", M2C_T_LAST_EXIT}, {"msa2_exit_s_1wave", M2C_T_EXIT1}, {"msa2_exit_s_4waves", M2C_T_EXIT4},
    {"msa2_exit_s_8waves", M2C_T_EXIT8},
    {"msa_bitvector_tile_bytes", M2_ELSEWHERE}, {"msa_bitvector_split", M2_ELSEWHERE}, {"msa_bitvector_redone", M2_ELSEWHERE},
    {"msa_host_plan_s", M2H_T_PLAN}, {"msa_host_upload_alloc_s", M2H_T_UPLOAD_ALLOC}, {"msa_host_pairwise_launch_s", M2H_T_PAIRWISE_LAUNCH},
    {"msa_host_rows_s", M2H_T_ROWS}, {"msa_host_select_s", M2_ELSEWHERE}, {"msa_host_total_s", M2H_T_TOTAL},
    {"msa_pairs_bitvector", M2_EVERY_ROUTE}, {"msa_pairs_packed", M2_EVERY_ROUTE}, {"msa_pairs_packed_linear", M2_EVERY_ROUTE},
    {"msa_pairs_int32", M2_EVERY_ROUTE}, {"msa_pairs_packed_c4", M2_EVERY_ROUTE}, {"msa_pairs_packed_c8", M2_EVERY_ROUTE},
    {"msa_pairs_packed_c16", M2_EVERY_ROUTE}, {"msa_pairs_int32_c4", M2_EVERY_ROUTE}, {"msa_pairs_int32_c8", M2_EVERY_ROUTE},
    {"msa_pairs_int32_c16", M2_EVERY_ROUTE}, {"msa_v1_fallback_weights", M2_EVERY_ROUTE},
};
static void m2_counts_reset(bool every_route) {
    for (const M2Count& r : m2_counts)
        if ((r.from == M2_EVERY_ROUTE) == every_route) ctx().counts[r.name] = 0;
}

double m2_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void m2_host_time(int part, double t0) {
    for (const M2Count& r : m2_counts)
        if (r.from == part) ctx().count_add(r.name, m2_now() - t0);
}

int M2Streams::ensure(int n) {
    if (device != ctx().device) {   // (streams and events belong to the device that was current when they were made)
        for (hipStream_t x : st) (void)hipStreamDestroy(x);
        for (hipEvent_t e : join) (void)hipEventDestroy(e);
        if (fork) (void)hipEventDestroy(fork);
        for (int k = 0; k < 2; ++k) { if (pair[k]) (void)hipEventDestroy(pair[k]); pair[k] = nullptr; }
        st.clear(); join.clear(); fork = nullptr;
        device = ctx().device;
    }
    if (!fork) SL_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k)
        if (!pair[k]) SL_HIP(hipEventCreateWithFlags(&pair[k], hipEventDisableTiming));
    while (static_cast<int>(st.size()) < n) {
        hipStream_t x; hipEvent_t e;
        SL_HIP(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
        SL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        st.push_back(x); join.push_back(e);
    }
    return 0;
}
M2Streams& m2_streams() { static M2Streams m; return m; }

// ---- a host pass over the groups by a few threads ----
static size_t m2_threads(bool little_work) {
    const unsigned hw = std::thread::hardware_concurrency();
    return little_work ? 1 : std::max<size_t>(1, std::min<size_t>(hw ? hw : 1, 8));
}
// fn(t, q0, q1) for the ranges [bounds[t], bounds[t + 1]) of groups: a thread each, a single range on the caller's
template <typename F>
static void m2_parallel(const std::vector<size_t>& bounds, F fn) {
    const size_t nt = bounds.size() - 1;
    if (nt == 1) { fn(size_t(0), bounds[0], bounds[1]); return; }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nt; ++t) pool.emplace_back(fn, t, bounds[t], bounds[t + 1]);
    for (std::thread& th : pool) th.join();
}

// Host tables of a batch: groups and members, and the band classes of the pairwise jobs (4.4 million at C4).  The offsets come
// from one serial pass over the groups; the members are then filled and the jobs counted by a few threads over disjoint ranges
// of groups.
static int m2_plan(M2Batch& B, const int64_t* grp_off, const int32_t* grp, const int64_t* rel, const long long* gsum, const int* gmx,
                   bool exact_w, int bandwidth) {
    const size_t ngr = B.ids.size();
    B.groups.assign(ngr, M2Group{});
    B.max_len = 0; B.max_wcap = 0; B.max_n = 0;
    long long map_pos = 0, col_pos = 0, pos_pos = 0, dist_pos = 0, ext_pos = 0, mem_pos = 0, job_pos = 0;
    for (size_t q = 0; q < ngr; ++q) {
        const int64_t g = B.ids[q];
        const int n = static_cast<int>(grp_off[g + 1] - grp_off[g]);
        M2Group& G = B.groups[q];
        G.first_member = static_cast<int>(mem_pos);
        G.n = n;
        const long long sum = gsum[B.slot[q]];   // sum and maximum of the group's read lengths (msa2_core)
        const int mx = gmx[B.slot[q]];
        const long long fast_w = m2_fast_width(n, mx);
        // (65535 columns is the ceiling of spec v2: positions and columns are 16-bit; only reachable when the sum of
        // the read lengths exceeds it AND the alignment really is that wide)
        // (msa2_max_columns: a lower ceiling, for the tests of the hand-over to spec v1)
        const long long ceiling = option(OPT_MSA2_MAX_COLUMNS) > 0 ? std::min(65535, option(OPT_MSA2_MAX_COLUMNS)) : 65535;
        G.wcap = static_cast<int>(std::min<long long>(ceiling, std::min<long long>(sum, exact_w ? sum : fast_w)));
        if (G.wcap < 1) G.wcap = 1;
        G.pos_base = pos_pos;
        G.first_job = job_pos;
        G.dist_base = dist_pos;
        G.ext_base = ext_pos;
        G.lmax = mx;
        G.map0 = map_pos;
        G.col0 = col_pos;
        pos_pos += static_cast<long long>(n) * G.wcap;
        dist_pos += static_cast<long long>(n) * n + n;
        ext_pos += static_cast<long long>(n) * (n - 1) / 2 * mx;
        map_pos += static_cast<long long>(std::max(0, n - 1)) * sum;
        col_pos += sum;
        mem_pos += n;
        job_pos += static_cast<long long>(n) * (n - 1) / 2;
        B.max_len = std::max(B.max_len, mx);
        B.max_wcap = std::max(B.max_wcap, G.wcap);
        B.max_n = std::max(B.max_n, n);
    }
    B.map_n = map_pos; B.col_n = col_pos; B.pos_n = pos_pos;
    B.ext_n = ext_pos;
    B.members.assign(static_cast<size_t>(mem_pos), M2Member{});
    B.member_group.assign(static_cast<size_t>(mem_pos), 0);
    B.njobs = static_cast<size_t>(job_pos);
    auto fill = [&](size_t q0, size_t q1, MsaJobSummary* sum) {
        for (size_t q = q0; q < q1; ++q) {
            const M2Group& G = B.groups[q];
            const int32_t* mem = grp + grp_off[B.ids[q]];
            const int n = G.n;
            M2Member* const M = B.members.data() + G.first_member;
            long long mp = G.map0, cp = G.col0;
            for (int a = 0; a < n; ++a) {
                M2Member& Me = M[a];
                Me.seq_off = rel[mem[a] - 1];
                Me.len = static_cast<int>(rel[mem[a]] - rel[mem[a] - 1]);
                Me.map_base = mp;
                Me.col_base = cp;
                Me.ext_base = G.ext_base; Me.first_member = G.first_member; Me.n = n; Me.lmax = G.lmax;
                mp += static_cast<long long>(std::max(0, n - 1)) * Me.len;
                cp += Me.len;
                B.member_group[static_cast<size_t>(G.first_member) + a] = static_cast<int>(q);
            }
            // band classes of the group's pairs (rows = b, columns = a: k_m2_jobs).  Where the longest and the shortest read of the
            // group already fit the narrow class -- nearly every group -- no pair needs a look of its own: the summary's sums
            // and maxima in closed form, the cell count from a branch-free loop.
            if (n < 2) continue;
            int lmin = M[0].len, lmax = M[0].len;
            for (int a = 1; a < n; ++a) { lmin = std::min(lmin, M[a].len); lmax = std::max(lmax, M[a].len); }
            const long long widest = static_cast<long long>(lmax - lmin) + 2LL * bandwidth + 1;
            if (widest <= 256) {
                sum->wide_listed = true;
                sum->n[0] += static_cast<size_t>(n) * (n - 1) / 2;
                sum->band[0] = std::max(sum->band[0], static_cast<int>(widest));
                const long long base = 2LL * bandwidth + 1;
                double cells = 0;
                for (int a = 0; a < n; ++a) {
                    const int la = M[a].len;
                    if (a + 1 < n) { sum->cols[0] += static_cast<double>(la) * (n - 1 - a); sum->lc[0] = std::max(sum->lc[0], la); }
                    if (a > 0) sum->lr[0] = std::max(sum->lr[0], la);
                    long long acc = 0;
                    for (int b = a + 1; b < n; ++b) { const long long lb = M[b].len; acc += lb * (base + (lb > la ? lb - la : la - lb)); }
                    cells += static_cast<double>(acc);
                }
                sum->cells += cells;
                continue;
            }
            long long j = G.first_job;
            for (int a = 0; a < n; ++a)
                for (int b = a + 1; b < n; ++b, ++j) sum->add(bandwidth, M[b].len, M[a].len, j);
        }
    };
    // ranges of groups with about the same number of jobs each
    const size_t nthreads = m2_threads(job_pos < 200000);
    std::vector<size_t> bounds(1, 0);
    for (size_t t = 0; t < nthreads; ++t) {
        const long long want = job_pos * static_cast<long long>(t + 1) / static_cast<long long>(nthreads);
        size_t q1 = bounds.back();
        while (q1 < ngr && (t + 1 == nthreads || B.groups[q1].first_job + static_cast<long long>(B.groups[q1].n) * (B.groups[q1].n - 1) / 2 <= want)) ++q1;
        bounds.push_back(q1);
    }
    std::vector<MsaJobSummary> part(nthreads);
    m2_parallel(bounds, [&](size_t t, size_t q0, size_t q1) { fill(q0, q1, &part[t]); });
    B.jsum = MsaJobSummary{};
    for (const MsaJobSummary& ps : part) B.jsum.merge(ps);
    return 0;
}

// reads, sum and maximum of the read lengths of every group of the list, once, by a few threads: the batch sizes and every
// batch's plan start from them (a serial pass over the 10^6 reads of C4 is 5 ms during which the device has nothing to run)
struct M2Sizes { std::vector<long long> n, sum; std::vector<int> mx; };
static M2Sizes m2_group_sizes(const int64_t* grp_off, const int32_t* grp, const std::vector<int64_t>& ids, const std::vector<int64_t>& rel) {
    M2Sizes S;
    S.n.resize(ids.size()); S.sum.resize(ids.size()); S.mx.resize(ids.size());
    const size_t nt = m2_threads(ids.size() < 20000);
    std::vector<size_t> bounds;
    for (size_t t = 0; t <= nt; ++t) bounds.push_back(ids.size() * t / nt);
    m2_parallel(bounds, [&](size_t, size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; ++q) {
            const int32_t* mem = grp + grp_off[ids[q]];
            const long long n = grp_off[ids[q] + 1] - grp_off[ids[q]];
            long long sum = 0, mx = 0;
            for (long long a = 0; a < n; ++a) { const long long len = rel[mem[a]] - rel[mem[a] - 1]; sum += len; mx = std::max(mx, len); }
            S.n[q] = n; S.sum[q] = sum; S.mx[q] = static_cast<int>(mx);
        }
    });
    return S;
}

// The cut of one pass's groups into batches: `todo` (indices into `ids` / S, by decreasing group size) -> the ids / slot lists
// of `batches`.  Returns the bytes the arrays of all the groups take together.  A function of its arguments: no device call.
struct M2Room {
    long long free_b, reusable;   // free device memory, and what the stage's own workspaces already hold
    long long mem_budget;         // bytes one batch may take
    int budget_gb, batches;       // the options msa2_budget_gb and msa2_batches
    bool unitw;
};
static long long m2_cut_batches(const std::vector<size_t>& todo, const std::vector<int64_t>& ids, const M2Sizes& S, bool exact_w,
                                const M2Room& R, std::vector<M2Batch>& batches) {
    const long long job_budget = 12000000;
    long long mem_all = 0, jobs_all = 0, ext_all = 0, cells_est = 0;
    std::vector<long long> cmem(todo.size() + 1, 0), cjobs(todo.size() + 1, 0);   // cumulative over the sorted list
    for (size_t x = 0; x < todo.size(); ++x) {
        const size_t q = todo[x];
        const long long n = S.n[q];
        const long long sum = S.sum[q], mx = S.mx[q];
        const long long wc = exact_w ? sum : std::min(sum, m2_fast_width(n, mx));
        mem_all += 2 * (n - 1) * sum + 2 * n * wc + 2 * sum + n * (n - 1) / 2 * mx * 4 * m2_ext_planes(R.unitw);
        ext_all += n * (n - 1) / 2 * mx * 4 * m2_ext_planes(R.unitw);
        cells_est += n * std::min(sum, 2 * mx);   // (rows: about the longest read, some more for clusters of several molecules)
        mem_all += n * (n - 1) / 2 * ((2 * mx) / 16 + 2) * 4;   // the move strings of the bit-vector pairwise kernel (msa_pairwise.hip)
        jobs_all += n * (n - 1) / 2;
        cmem[x + 1] = mem_all; cjobs[x + 1] = jobs_all;
    }
    // batches: as many as memory and the job list demand, a few more for the overlap once there is enough work.  (Until round 5
    // every batch got every nb-th group of the sorted list, "the same mix of sizes" -- and so every batch held some of the
    // largest groups, whose merging is the longest chain of dependent joins of the call: a 64-read cluster keeps its workgroup
    // busy for about 2 s, and the merge stage of a call took nb x that -- the same clusters in 1 / 3 / 5 batches: 2.96 / 6.6 /
    // 9.6 s.  Now the LARGE groups go to the batches in contiguous pieces of the sorted list -- the largest share the first
    // batch, the longest group of every later batch is shorter than that of the one before -- and only the bulk of
    // one-wavefront groups is dealt round robin.)
    // (one batch when everything fits -- then the stage timers do not overlap either; from two on the two workspace
    // sets share the budget.  Measured at C4 with two pipelined batches: pure groups 5 % faster end to end, clusters
    // of several molecules unchanged -- the alignments saturate the vector units by themselves.)
    long long nb = std::max<long long>(1, std::max((mem_all + R.mem_budget - 1) / R.mem_budget, (jobs_all + job_budget - 1) / job_budget));
    // One batch whenever the device holds it: what the stage needs beside a batch's arrays is bounded -- the tile buffer of the
    // alignments (48 GB at most, and it doubles as plane 0 of the extended library), the per-workgroup scratch of the merging
    // (16 GB per class at most), the rows.  (Until the library was stored, a batch could have half of what was free and
    // bench.py's pipeline workload fitted; with it the half-rule cut that call into 4 batches and the merging's launches, each
    // as long as its longest group, into 4 rounds: 647 ms against 420.)
    bool one_batch = false;
    if (R.budget_gb <= 0 && R.batches <= 1 && jobs_all <= job_budget) {
        const long long plane0 = ext_all / m2_ext_planes(R.unitw);
        const long long rows_est = 2 * cells_est;
        const long long extra = std::max<long long>(48LL << 30, plane0) - plane0 + (48LL << 30) + rows_est + (8LL << 30);
        one_batch = mem_all + extra <= R.free_b + R.reusable;
        if (one_batch) nb = 1;
    }
    const long long want = R.batches > 0 ? R.batches : 1;
    if (!one_batch && std::max(nb, want) > 1) nb = std::max<long long>(want, std::max((2 * mem_all + R.mem_budget - 1) / R.mem_budget, (jobs_all + job_budget - 1) / job_budget));
    nb = std::min<long long>(nb, static_cast<long long>(todo.size()));
    batches.assign(static_cast<size_t>(nb), M2Batch{});
    // groups of more than M2_NB reads (several wavefronts each, the long chains of joins): contiguous pieces of the sorted
    // list, by their share of the memory and of the jobs of all such groups; the rest: every nb-th group, so that every
    // batch has the same bulk of one-wavefront groups to fill the chip beside its large ones
    size_t nbig = 0;
    while (nbig < todo.size() && S.n[todo[nbig]] > M2_NB) ++nbig;
    const long long bmem = cmem[nbig], bjobs = cjobs[nbig];
    size_t k = 0;
    for (size_t x = 0; x < nbig; ++x) {
        const double share = std::max(bmem > 0 ? static_cast<double>(cmem[x]) / static_cast<double>(bmem) : 0.0,
                                      bjobs > 0 ? static_cast<double>(cjobs[x]) / static_cast<double>(bjobs) : 0.0);
        while (k + 1 < static_cast<size_t>(nb) && share * static_cast<double>(nb) >= static_cast<double>(k + 1)) ++k;
        batches[k].ids.push_back(ids[todo[x]]);
        batches[k].slot.push_back(todo[x]);
    }
    for (size_t x = nbig; x < todo.size(); ++x) {
        M2Batch& B = batches[(x - nbig) % static_cast<size_t>(nb)];
        B.ids.push_back(ids[todo[x]]);
        B.slot.push_back(todo[x]);
    }
    // (a call with fewer groups than batches, or one huge group taking the share of two pieces, leaves a batch without groups)
    batches.erase(std::remove_if(batches.begin(), batches.end(), [](const M2Batch& B) { return B.ids.empty(); }), batches.end());
    return mem_all;
}

// row buffer ("msa2.rows"): grown when a batch does not fit (contents, `used` bytes, are kept)
static int m2_rows_reserve(Workspace& rows_ws, size_t used, size_t need, hipStream_t s) {
    if (rows_ws.cap >= need) return 0;
    const size_t want = std::max(need, rows_ws.cap + rows_ws.cap / 2) + 4096;
    void* np = nullptr;
    if (hipMalloc(&np, want) != hipSuccess) {
        size_t fb = 0, tb = 0;
        (void)hipGetLastError();
        (void)hipMemGetInfo(&fb, &tb);
        size_t held = 0;
        for (const auto& kv : ctx().ws) held += kv.second.cap;
        return fail("sarlacc_amd: cannot allocate %zu bytes of device memory for the alignment rows (%zu free of %zu, the library's workspaces hold %zu)", want, fb, tb, held);
    }
    if (rows_ws.ptr) {
        if (used) SL_HIP(hipMemcpyAsync(np, rows_ws.ptr, used, hipMemcpyDeviceToDevice, s));
        SL_HIP(hipStreamSynchronize(s));
        SL_HIP(hipFree(rows_ws.ptr));
    }
    rows_ws.ptr = np;
    rows_ws.cap = want;
    return 0;
}

// spec v2 on the groups `ids` of the caller's list; rows land in *d_rows at off[k] for ids[k] (processing order:
// the offsets are not cumulative in k), widths in width[k].
static int msa2_core(const int64_t* grp_off, const int32_t* grp, const std::vector<int64_t>& ids, const uint8_t* d_seq,
                     const std::vector<int64_t>& rel, double match, double mismatch, double gap_extension, double gap_opening,
                     int bandwidth, std::vector<int32_t>& width, std::vector<long long>& off, uint8_t** d_rows,
                     const std::function<int()>* overlap, const CodeSpec& code, hipStream_t s, std::vector<size_t>* gave_up) {
    Context& c = ctx();
    const size_t cs = code.want ? 2 : 1;   // bytes per cell of the row buffer (offsets and widths stay in cells)
    bool waited = false;
    width.assign(ids.size(), 0);
    off.assign(ids.size() + 1, 0);
    *d_rows = nullptr;
    Workspace& rows_ws = c.ws["msa2.rows"];
    // Batches.  What a batch holds per group is the library (both maps of every pair: 4 (n - 1) bytes per base), the positions /
    // columns of its profiles and the extended library (12 or 16 bytes per pair and position) -- about 165 GB for C4 (10^5 groups x 10 reads
    // x 2 kb), sized for an HBM of 288 GB and bounded by a share of what is free now.  A large call is cut into a few
    // batches that are PIPELINED: the all-pairs alignments of batch k + 1 (vector-unit bound) run on a stream of their
    // own under the merging of batch k (memory-latency bound); two sets of workspaces alternate.
    size_t free_b = 0, total_b = 0;
    SL_HIP(hipMemGetInfo(&free_b, &total_b));
    // the workspaces an earlier call left are grown in place, not added: everything this stage holds -- the batches' maps, positions,
    // columns and tables, but also the pairwise kernel's traceback records and move strings, the merging's per-workgroup scratch and
    // the rows (counting only the first four made the SECOND of two equal calls see half the room and cut itself into 5 batches
    // where the first took 3)
    long long reusable = 0;
    for (const auto& kv : c.ws)
        if (kv.first.compare(0, 2, "m2") == 0 || kv.first.compare(0, 4, "msa.") == 0 || kv.first.compare(0, 5, "msa2.") == 0)
            reusable += static_cast<long long>(kv.second.cap);
    // (msa2_budget_gb: the cap in GB, tests and sweeps; the default leaves the other half of what is free to the traceback records of
    // the pairwise kernel, the per-workgroup scratch of the merging and the rows)
    const long long budget_cap = option(OPT_MSA2_BUDGET_GB) > 0 ? static_cast<long long>(option(OPT_MSA2_BUDGET_GB)) << 30 : 96LL << 30;
    const long long mem_budget = std::max<long long>(1LL << 30, std::min<long long>(budget_cap, (static_cast<long long>(free_b) + reusable) / 2));
    const M2Room room = {static_cast<long long>(free_b), reusable, mem_budget, option(OPT_MSA2_BUDGET_GB), option(OPT_MSA2_BATCHES),
                         m2_unit_weights(static_cast<int>(match), static_cast<int>(mismatch))};
    // the call's values: [M2C_*] summed over the batches by m2_merge, [M2H_*] counted here -- pairs and cells of the alignments,
    // groups whose profiles outgrew the first-pass capacity, batches (from two on the stage timers of alignments and merging overlap)
    double v[M2H_VALUES] = {};
    long long used = 0;
    M2Streams& MS = m2_streams();
    SL_TRY(MS.ensure(3));
    hipStream_t sp = MS.st[2];
    SL_HIP(hipEventRecord(MS.fork, s));          // whatever the caller queued on `s` (the reads) comes first
    SL_HIP(hipStreamWaitEvent(sp, MS.fork, 0));
    bool first = true;
    // Pass 0: every group with the fast profile capacity.  Pass 1: the groups whose profiles outgrew it (several
    // unrelated reads in one cluster), with profiles as wide as the sum of the read lengths.
    std::vector<size_t> todo(ids.size());
    std::iota(todo.begin(), todo.end(), size_t(0));
    const M2Sizes S = m2_group_sizes(grp_off, grp, ids, rel);
    for (int pass = 0; pass < 2 && !todo.empty(); ++pass) {
        const bool exact_w = pass == 1;
        // processing order: by decreasing group size -- the workgroups of k_m2_group take the groups in this order, the
        // longest first
        std::stable_sort(todo.begin(), todo.end(), [&](size_t x, size_t y) { return S.n[x] > S.n[y]; });
        std::vector<size_t> again;
        std::vector<M2Batch> batches;
        const long long mem_all = m2_cut_batches(todo, ids, S, exact_w, room, batches);
        c.counts["msa2_mem_all_gb"] = static_cast<double>(mem_all) / 1073741824.0;
        c.counts["msa2_mem_budget_gb"] = static_cast<double>(mem_budget) / 1073741824.0;
        v[M2H_BATCHES] += static_cast<double>(batches.size());
        // the pipeline: prepare(k + 1), m2_merge(k), the row layout, m2_write_batch(k)
        const char* const pfs[2] = {"m2a", "m2b"};
        auto prepare = [&](size_t k) -> int {
            M2Batch& B = batches[k];
            double th = m2_now();
            SL_TRY(m2_plan(B, grp_off, grp, rel.data(), S.sum.data(), S.mx.data(), exact_w, bandwidth));
            m2_host_time(M2H_T_PLAN, th);
            B.pair_done = MS.pair[k & 1];
            B.alias_tiles = batches.size() == 1;
            SL_TRY(m2_prepare(B, pfs[k & 1], d_seq, match, mismatch, gap_extension, gap_opening, bandwidth, &v[M2H_CELLS], first, sp));
            v[M2H_PAIRS] += static_cast<double>(B.njobs);
            if (first && overlap) SL_TRY((*overlap)());
            first = false;
            return 0;
        };
        SL_TRY(prepare(0));
        for (size_t k = 0; k < batches.size(); ++k) {
            M2Batch& B = batches[k];
            if (k + 1 < batches.size()) SL_TRY(prepare(k + 1));   // (its workspaces: those of batch k - 1, finished and read back)
            SL_TRY(m2_merge(B, pfs[k & 1], v, s));
            double th = m2_now();
            long long need = used;
            std::vector<long long> boff(B.groups.size(), 0);
            std::vector<int32_t> bw = B.width;
            // The rows of a batch are laid out in the CALLER's group order (the batch itself is ordered by group size): when one
            // batch holds every group -- the usual case -- the buffer is then already what msa_run hands on, and its gathering
            // copy (4.6 GB of vote codes at 10^6 reads: 5 ms) is skipped.
            std::vector<size_t> byslot(B.groups.size());
            std::iota(byslot.begin(), byslot.end(), size_t(0));
            std::sort(byslot.begin(), byslot.end(), [&](size_t x, size_t y) { return B.slot[x] < B.slot[y]; });
            for (size_t q : byslot) {
                if (B.ovf[q]) {   // profile capacity exceeded: next pass
                    // (with profiles as wide as 16-bit columns allow and still too narrow: the alignment is wider than 65 535 columns,
                    // beyond spec v2 -- the caller hands the group to spec v1)
                    if (exact_w) gave_up->push_back(B.slot[q]); else again.push_back(B.slot[q]);
                    bw[q] = 0;
                    continue;
                }
                width[B.slot[q]] = bw[q];
                off[B.slot[q]] = need;
                boff[q] = need;
                need += static_cast<long long>(bw[q]) * B.groups[q].n;
            }
            SL_TRY(m2_rows_reserve(rows_ws, static_cast<size_t>(used) * cs, (static_cast<size_t>(need) + 1) * cs, s));
            SL_HIP(hipMemcpyAsync(B.a.width, bw.data(), sizeof(int32_t) * bw.size(), hipMemcpyHostToDevice, s));
            B.width = bw;
            if (code.want && code.ready && !waited) { SL_HIP(hipStreamWaitEvent(s, code.ready, 0)); waited = true; }   // qualities in HBM
            SL_TRY(m2_write_batch(B, pfs[k & 1], boff, rows_ws.ptr, code, s));
            SL_HIP(hipStreamSynchronize(s));   // the batch's host vectors and workspaces are reused by the batch after the next
            m2_host_time(M2H_T_ROWS, th);
            used = need;
        }
        if (pass == 0) v[M2H_SECOND_PASS] = static_cast<double>(again.size());
        todo.swap(again);
    }
    SL_HIP(hipStreamSynchronize(sp));
    if (v[M2H_PAIRS] > 0) {
        int* d_stuck;
        int stuck = 0;
        SL_TRY(scratch("msa.stuck", 1, &d_stuck));
        SL_HIP(hipMemcpy(&stuck, d_stuck, sizeof stuck, hipMemcpyDeviceToHost));
        if (stuck) return fail("sarlacc_amd: internal error: an MSA traceback exceeded its step bound");
    }
    for (const M2Count& r : m2_counts)
        if (r.from >= 0 && r.from < M2H_VALUES) c.count_add(r.name, v[r.from]);
    if (!rows_ws.ptr) SL_TRY(m2_rows_reserve(rows_ws, 0, 16, s));
    *d_rows = static_cast<uint8_t*>(rows_ws.ptr);
    return 0;
}

// Scoring domain of the MSA stage (oracle/oracle.py msa_check_scores states the same rule).  The four
// scores are truncated toward zero to integers.  With S the largest magnitude among them and L the longest read of the call's
// groups, the call is accepted when  S * (2 L + 2) < 2^27:
//   * every finite cell of a pairwise DP is a sum of at most lr + lc <= 2 L scores, so |H|, |E|, |F| <= S (lr + lc);
//   * the 32-bit kernel (msa_pairwise.hip) stands for "outside the band" by MSA_NEG = -2^28 PLUS what the recurrence adds to it
//     (a cell beyond the band edge holds a finite value of that size, one penalty is added on the way in), i.e. at most
//     -2^28 + S (lr + lc + 2).  That has to stay below every finite candidate, which is at least -S (lr + lc + 2):
//     2 S (lr + lc + 2) < 2^28.  The CPU statement's "outside" is the constant INT_MIN / 4 = -2^29, never added to: the looser of
//     the two, so the kernel's bound decides;
//   * no 32-bit sum overflows (2^28 + 2^28 + 2^27 < 2^31), and |score| < 2^27 makes the conversion from double defined
//     (NaN and infinities fail the comparison and are rejected with the rest).
static int msa_check_scores(double match, double mismatch, double gap_extension, double gap_opening, int64_t longest) {
    const double lim = 134217728.0;   // 2^27
    long long smax = 0;
    for (const double v : {match, mismatch, gap_extension, gap_opening}) {
        if (!(std::fabs(v) < lim)) { smax = 1LL << 27; break; }
        smax = std::max(smax, std::llabs(static_cast<long long>(v)));
    }
    if (smax * (2 * static_cast<long long>(longest) + 2) >= (1LL << 27))
        return fail("sarlacc_amd: MSA scores outside the scoring domain: max |score| * (2 * longest read + 2) must stay below 2^27 "
                    "(scores %g %g %g %g, longest read %lld)", match, mismatch, gap_extension, gap_opening, static_cast<long long>(longest));
    return 0;
}

// Spec v2 with weights other than 1: does a group of n reads, the longest of `longest` bases, under
// the largest primary weight W = max(match, mismatch, 1) fit the fields its weights are kept in?  With P = floor(n/2) ceil(n/2),
// the most member pairs (a, b) a join of two profiles can have:
//   * a library record of (a, p, b) sums the direct weight and one triplet per third read, (n - 1) W at most, into the 16 bits
//     of its slot (k_m2_extend: w0 | others << 16, wk | qk << 16):                               (n - 1) W <= 65 535;
//   * a row entry sums one slot of the record of every member pair, P (n - 1) W at most, in a 32-bit int that the noise
//     filter doubles (2 w >= heaviest):                                                          P (n - 1) W < 2^30
//     (implied by the first bound, 1 024 * 65 535 < 2^30; stated because the field is a different one);
//   * a chain sums row entries in 32 unsigned bits ((f << 32) | ~id).  Every position p of a member a lies in ONE column of the
//     first child, hence in at most one match of a chain, where the pair (a, b) adds one slot of its record:
//                                                                                         P (n - 1) W longest <= 2^32 - 1.
// With W = 1 all three hold for every group spec v2 takes (n <= 64, longest <= 65 471: 1 024 * 63 * 65 471 < 2^32), so the
// unit-weight path never sees the guard act.
static bool m2_weights_fit(long long n, long long longest, long long W) {
    if (n < 2) return true;
    const long long P = (n / 2) * ((n + 1) / 2), rec = (n - 1) * W;
    if (rec > 65535) return false;
    return P * rec < (1LL << 30) && P * rec * longest <= 0xFFFFFFFFLL;
}

// The MSA stage of quick_msa: spec v2 for groups of up to M2_MAXN reads whose profiles fit 65535 columns,
// spec v1 (msa.hip) for the rest and when spec 1 is selected (sarlacc_set_msa_spec / SARLACC_MSA_SPEC=1).
int msa_run(const int64_t* grp_off, const int32_t* grp, int64_t ngroups, const char* seq, const int64_t* seq_off,
            int64_t nseq, double match, double mismatch, double gap_extension, double gap_opening, int bandwidth,
            bool want_rows, int64_t out_cap, MsaResult* res, const std::function<int()>* overlap,
            const uint8_t* d_seq_resident) {
    {   // the scoring domain, on every route into the stage (both specs, rows or fused, host or resident reads)
        int64_t longest = 0;
        for (int64_t k = grp_off[0]; k < grp_off[ngroups]; ++k)
            if (grp[k] >= 1 && grp[k] <= nseq) longest = std::max<int64_t>(longest, seq_off[grp[k]] - seq_off[grp[k] - 1]);
        SL_TRY(msa_check_scores(match, mismatch, gap_extension, gap_opening, longest));
        m2_counts_reset(true);
    }
    if (msa_spec() == 1)
        return msa1_run(grp_off, grp, ngroups, seq, seq_off, nseq, match, mismatch, gap_extension, gap_opening, bandwidth, want_rows,
                        out_cap, res, overlap, d_seq_resident);
    int32_t* width_out = res->width.data();
    int64_t* out_off = res->out_off.data();
    res->d_out = nullptr;
    res->d_members = nullptr;
    out_off[0] = 0;
    if (bandwidth < 0) return fail("sarlacc_amd: negative bandwidth");
    const int64_t nmemb = grp_off[ngroups] - grp_off[0];
    for (int64_t i = 0; i < nmemb; ++i) {
        const int32_t v = grp[grp_off[0] + i];
        if (v < 1 || v > nseq) return fail("sarlacc_amd: group index %d outside 1..%lld", v, static_cast<long long>(nseq));
    }
    std::vector<int64_t> rel(static_cast<size_t>(nseq) + 1);
    for (int64_t i = 0; i <= nseq; ++i) rel[i] = (nseq ? seq_off[i] : 0) - (nseq ? seq_off[0] : 0);
    // which groups does spec v2 take
    std::vector<int64_t> v2, v1;
    const long long wmax = std::max(1LL, std::max(static_cast<long long>(match), static_cast<long long>(mismatch)));   // as truncated
    double diverted_weights = 0;
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t n = grp_off[g + 1] - grp_off[g];
        int64_t mx = 0;
        for (int64_t a = 0; a < n; ++a) { const int32_t id = grp[grp_off[g] + a]; mx = std::max<int64_t>(mx, rel[id] - rel[id - 1]); }
        if (mx > 60000) return fail("sarlacc_amd: reads longer than 60000 bases are not supported by the MSA stage");
        // spec v2: up to M2_MAXN reads, each short enough for 16-bit positions (a profile that outgrows 65 535 COLUMNS sends its group
        // to spec v1 afterwards: msa2_core's gave_up)
        // ... and with weights that fit the fields of the library records, the rows and the chain (m2_weights_fit)
        const bool v2_shape = n <= M2_MAXN && mx + 64 <= 65535;
        const bool fit = !v2_shape || m2_weights_fit(n, mx, wmax);
        if (!fit) diverted_weights += 1;
        if (v2_shape && fit) v2.push_back(g); else v1.push_back(g);
    }
    ctx().counts["msa_v1_fallback_weights"] = diverted_weights;
    SL_TRY(ensure_device());
    Context& c = ctx();
    hipStream_t s = nullptr;
    c.stage_reset("msa_pairwise");
    c.stage_reset("msa_merge");
    m2_counts_reset(false);
    const double t_run = m2_now();
    if (v2.empty())
        return msa1_run(grp_off, grp, ngroups, seq, seq_off, nseq, match, mismatch, gap_extension, gap_opening, bandwidth, want_rows,
                        out_cap, res, overlap, d_seq_resident);
    const int64_t total = rel[nseq];
    uint8_t* d_seq;
    if (d_seq_resident) d_seq = const_cast<uint8_t*>(d_seq_resident);
    else SL_TRY(upload("msa.seq", reinterpret_cast<const uint8_t*>(seq) + (nseq ? seq_off[0] : 0), static_cast<size_t>(total), &d_seq, s));
    int32_t* d_mem;
    SL_TRY(upload("msa.mem.all", grp + grp_off[0], static_cast<size_t>(nmemb), &d_mem, s));   // (msa1_run uploads its own "msa.mem")
    res->d_members = d_mem;

    std::vector<int32_t> w2;
    std::vector<long long> o2;
    uint8_t* d_rows2 = nullptr;
    std::vector<size_t> gave_up;
    SL_TRY(msa2_core(grp_off, grp, v2, d_seq, rel, match, mismatch, gap_extension, gap_opening, bandwidth, w2, o2, &d_rows2, overlap, res->code, s, &gave_up));
    if (!gave_up.empty()) {   // alignments wider than 65 535 columns: spec v1 (the list stays in group order)
        for (size_t q : gave_up) v1.push_back(v2[q]);
        std::sort(v1.begin(), v1.end());
    }
    c.counts["msa_v1_fallback"] = static_cast<double>(v1.size());
    c.counts["msa_v1_fallback_too_wide"] = static_cast<double>(gave_up.size());
    // spec v1 part on a compacted group list: more than M2_MAXN reads, reads too long, or dropped by the guard
    MsaResult r1;
    std::vector<int64_t> g1off(v1.size() + 1, 0);
    std::vector<int32_t> g1;
    if (!v1.empty()) {
        for (size_t q = 0; q < v1.size(); ++q) {
            const int64_t g = v1[q];
            for (int64_t k = grp_off[g]; k < grp_off[g + 1]; ++k) g1.push_back(grp[k]);
            g1off[q + 1] = static_cast<int64_t>(g1.size());
        }
        r1.width.assign(v1.size(), 0);
        r1.out_off.assign(v1.size() + 1, 0);
        r1.code = res->code;
        SL_TRY(msa1_run(g1off.data(), g1.data(), static_cast<int64_t>(v1.size()), seq, seq_off, nseq, match, mismatch, gap_extension,
                        gap_opening, bandwidth, true, -1, &r1, nullptr, d_seq, true));
    }
    // the rows of spec v2 are in processing order, those of spec v1 in a buffer of their own: gather both into one in group order
    std::vector<long long> src_off(static_cast<size_t>(ngroups)), dst_off(static_cast<size_t>(ngroups)), nbytes(static_cast<size_t>(ngroups));
    std::vector<char> from1(static_cast<size_t>(ngroups), 0);
    {
        size_t a1 = 0, a2 = 0;
        for (int64_t g = 0; g < ngroups; ++g) {
            const int64_t n = grp_off[g + 1] - grp_off[g];
            const bool in2 = a2 < v2.size() && v2[a2] == g;
            if (a1 < v1.size() && v1[a1] == g) { width_out[g] = r1.width[a1]; src_off[g] = r1.out_off[a1]; from1[g] = 1; ++a1; }
            else { width_out[g] = w2[a2]; src_off[g] = o2[a2]; }
            if (in2) ++a2;
            nbytes[g] = static_cast<long long>(width_out[g]) * n;
            dst_off[g] = out_off[g];
            out_off[g + 1] = out_off[g] + nbytes[g];
        }
    }
    if (want_rows && out_cap >= 0 && out_cap < out_off[ngroups]) return fail("sarlacc_amd: MSA output buffer too small (%lld needed)", static_cast<long long>(out_off[ngroups]));
    // spec v2's buffer already in group order (one batch, no group by spec v1, none that needed the second pass): it IS the result
    bool in_place = v1.empty();
    for (int64_t g = 0; g < ngroups && in_place; ++g) in_place = src_off[g] == dst_off[g];
    if (in_place) {
        SL_HIP(hipStreamSynchronize(s));
        if (res->code.want) res->d_codes = reinterpret_cast<uint16_t*>(d_rows2);
        else res->d_out = d_rows2;
        m2_host_time(M2H_T_TOTAL, t_run);
        return 0;
    }
    // (offsets and sizes so far are in cells; a cell is one character, or one 16-bit vote code)
    const long long cs = res->code.want ? 2 : 1;
    uint8_t* d_final;
    SL_TRY(scratch(res->code.want ? "msa.final16" : "msa.final", static_cast<size_t>(out_off[ngroups] * cs) + 8, &d_final));
    if (cs > 1)
        for (int64_t g = 0; g < ngroups; ++g) { src_off[g] *= cs; dst_off[g] *= cs; nbytes[g] *= cs; }
    const uint8_t* src1 = res->code.want ? reinterpret_cast<const uint8_t*>(r1.d_codes) : r1.d_out;
    SL_TRY(msa_rows_gather(src1, d_rows2, src_off, dst_off, nbytes, from1, !v1.empty(), d_final, s));
    SL_HIP(hipStreamSynchronize(s));
    if (res->code.want) res->d_codes = reinterpret_cast<uint16_t*>(d_final);
    else res->d_out = d_final;
    m2_host_time(M2H_T_TOTAL, t_run);
    return 0;
}

}  // namespace sarlacc

using namespace sarlacc;

extern "C" int sarlacc_set_msa_spec(int spec) {
    if (spec != 0 && spec != 1 && spec != 2) return fail("sarlacc_amd: MSA spec must be 1 (centre-star) or 2 (consistency-based progressive), 0 = default");
    return sarlacc::set_option("msa_spec", spec);
}
