// profile_reads.hip -- the profiling workflow on resident reads: align every read to its reference (run_align, strings),
// then reduce the alignments to the error profile and the homopolymer profile where the aligner left them.  Stands for
// the chain general_align -> find_errors + match_homopolymers (the reference's src/general_align.cpp:10-62,
// src/find_errors.cpp:9-121, src/homopolymer.cpp:141-209) without a string or a per-event list leaving the device.
//
// k_profile_pairs reads the aligner's slots AS THEY ARE: end-first, slot of read i at off[i] + i * R.  ONE WAVEFRONT PER
// ALIGNMENT, 64 characters per step, from slot index 0 up -- that is from the alignment's END to its start.  Every
// quantity of the forward routines has a mirror image, so nothing is reversed or copied:
//   * the reference base at a column is number R - 1 - (reference bases met so far);
//   * a run of reference gaps (an insertion) is filed under the NEXT reference base of the forward string, which this
//     walk has met BEFORE the run: position = R - (reference bases met so far), R for a run at the forward end.  A run
//     is emitted where it ends (the first reference base after it, or the end of the slot), and only its length so far
//     is carried from step to step;
//   * the runs of the mirrored reference are the mirrored runs, and "the longest run of the same base in the read that
//     overlaps it" is symmetric, so pf_runs (profile_walk.hpp) and the walk of k_match_homopolymers apply unchanged; a
//     run that starts at mirrored position p with l bases is the forward run starting at R - p - l (a table from the
//     host names it).
// Counts per reference position are kept in LDS by the workgroup over all the alignments it walks (a persistent grid)
// and flushed once: 5 x PR_TILE counters; a longer reference is tiled over blockIdx.y, tile 0 also emitting the events.
// Events go into dense tables (position x length, run x length) for lengths below PR_DENSE and into a list beyond;
// after the last chunk the occupied cells and the list are sorted together and merged (rocPRIM), which leaves the
// distinct pairs in ascending order with their multiplicities.
#include "align_host.hpp"
#include "common.hpp"
#include "devprim.hpp"
#include "profile_walk.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

namespace sarlacc {

constexpr int PR_WAVES = 8;      // alignments a workgroup walks at a time
constexpr int PR_TILE = 2048;    // reference positions whose counters a workgroup keeps in LDS (5 x 2048 x 4 B = 40 KB)
constexpr int PR_DENSE = 64;     // event lengths below this are counted in a dense table

// one kind of event: (row, length) with row = reference position (insertions) or run index (homopolymer observations)
struct PrEvents {
    int* dense;                   // [rows][PR_DENSE]
    unsigned long long* list;     // row << 32 | length, for lengths from PR_DENSE on
    unsigned long long* used;     // entries of the list asked for so far
    long long cap;
};

struct PrArgs {
    const uint8_t* aln_ref;
    const uint8_t* aln_qry;
    const int32_t* aln_len;
    const int64_t* off;           // offsets of this chunk's reads (slot of read i at off[i] - off[0] + i * R)
    long long n, read_base;       // reads in the chunk, index of its first read in the call
    int R, nruns;
    const int32_t* run_of;        // [R] index of the run that starts at a reference position, -1 elsewhere
    int* counts;                  // [5][R]
    PrEvents ins, obs;
    unsigned long long* first_bad;   // minimum of alignment << 32 | forward position of an unknown read character
    int* trouble;                 // 1: a list overflowed, 2: an alignment does not spell the reference
};

__device__ __forceinline__ void pr_event(const PrEvents& e, int* trouble, long long row, long long len) {
    if (len < PR_DENSE) {
        atomicAdd(&e.dense[row * PR_DENSE + len], 1);
    } else {
        const unsigned long long o = atomicAdd(e.used, 1ull);
        if (o < static_cast<unsigned long long>(e.cap)) e.list[o] = (static_cast<unsigned long long>(row) << 32) | static_cast<unsigned long long>(len);
        else atomicMax(trouble, 1);
    }
}

__global__ void __launch_bounds__(64 * PR_WAVES) k_profile_pairs(PrArgs A) {
    __shared__ int cnt[5 * PR_TILE];
    for (int k = threadIdx.x; k < 5 * PR_TILE; k += 64 * PR_WAVES) cnt[k] = 0;
    __syncthreads();
    const int lane = pf_lane();
    const long long tile_lo = static_cast<long long>(blockIdx.y) * PR_TILE;
    const bool events = blockIdx.y == 0;
    const long long off0 = A.off[0];
    for (long long i = blockIdx.x * static_cast<long long>(PR_WAVES) + (threadIdx.x >> 6); i < A.n; i += static_cast<long long>(gridDim.x) * PR_WAVES) {
        const long long base = A.off[i] - off0 + i * A.R;
        const uint8_t* const rf = A.aln_ref + base;
        const uint8_t* const rd = A.aln_qry + base;
        const long long len = A.aln_len[i];
        long long met = 0, gaprun = 0;   // reference bases met so far; reference gaps at the end of what was seen
        for (long long x0 = 0; x0 < len; x0 += 64) {
            const long long x = x0 + lane;
            const bool in = x < len;
            const int rc = in ? rf[x] : 'A';
            const bool ng = in && rc != '-';
            const unsigned long long m_ng = __ballot(ng), m_in = __ballot(in);
            const long long before = met + __popcll(m_ng & pf_below(lane));
            if (ng) {
                const long long t = A.R - 1 - before - tile_lo;   // (every reference position lies in exactly one tile)
                if (t >= 0 && t < PR_TILE) {
                    int kind;
                    switch (rd[x]) {
                        case 'A': kind = 0; break;
                        case 'C': kind = 1; break;
                        case 'G': kind = 2; break;
                        case 'T': kind = 3; break;
                        case '-': kind = 4; break;
                        default: kind = -1; break;
                    }
                    if (kind >= 0) atomicAdd(&cnt[kind * PR_TILE + t], 1);
                    else atomicMin(A.first_bad, (static_cast<unsigned long long>(A.read_base + i) << 32) | static_cast<unsigned long long>(len - 1 - x));
                } else if (t < 0 && events) {
                    atomicMax(A.trouble, 2);
                }
            }
            if (events) {
                const int pl = pf_prev(m_ng, lane);
                const long long glen = pl < 0 ? gaprun + lane : lane - pl - 1;
                if (ng && glen > 0 && before <= A.R) pr_event(A.ins, A.trouble, A.R - before, glen);
                const int nin = __popcll(m_in);
                if (m_ng) gaprun = nin - (63 - __builtin_clzll(m_ng)) - 1; else gaprun += nin;
            }
            met += __popcll(m_ng);
            if (!events && A.R - 1 - met < tile_lo) break;   // the rest lies below this tile
        }
        if (!events) continue;
        if (met != A.R) { if (lane == 0) atomicMax(A.trouble, 2); continue; }
        if (gaprun > 0 && lane == 0) pr_event(A.ins, A.trouble, A.R - met, gaprun);   // gaps at the forward start
        if (A.nruns == 0) continue;
        pf_runs(rf, len, [&](bool fire, long long left, long long far_right, long long rpos, long long rl, int rbase, long long far_left, long long right) {
            if (!fire || rl < 2) return;
            // as in k_match_homopolymers: the read over the reference run extended by the gaps on either side
            long long best = 0, qs = 0, qe = 0, ql = 0;
            int qb = 0;
            for (long long x = far_left; x <= far_right; ++x) {
                const int c = x < far_right ? rd[x] : 0;     // 0 closes the last run
                if (c == '-') continue;
                if (c != qb) {
                    if (qb != 0 && qb == rbase && right > qs && left < qe && ql > best) best = ql;
                    qb = c; qs = x; ql = 0;
                }
                ++ql; qe = x + 1;
            }
            const long long start = A.R - rpos - rl;
            const int run = start >= 0 && start < A.R ? A.run_of[start] : -1;
            if (run >= 0) pr_event(A.obs, A.trouble, run, best);
            else atomicMax(A.trouble, 2);
        });
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 5 * PR_TILE; k += 64 * PR_WAVES) {
        const int kind = k / PR_TILE;
        const long long p = tile_lo + (k - kind * PR_TILE);
        if (p < A.R && cnt[k]) atomicAdd(&A.counts[static_cast<long long>(kind) * A.R + p], cnt[k]);
    }
}

// occupied cells of a dense table as (row << 32 | length, count): WRITE = false counts them
template <bool WRITE>
__global__ void k_pr_cells(const int* dense, long long ncells, unsigned long long* used, unsigned long long* keys, long long* mult) {
    const long long c = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (c >= ncells) return;
    const int v = dense[c];
    if (v == 0) return;
    const unsigned long long o = atomicAdd(used, 1ull);
    if (WRITE) {
        keys[o] = (static_cast<unsigned long long>(c / PR_DENSE) << 32) | static_cast<unsigned long long>(c % PR_DENSE);
        mult[o] = v;
    }
}

__global__ void k_pr_ones(long long* mult, long long n) {
    const long long k = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (k < n) mult[k] = 1;
}

__global__ void k_pr_split(const unsigned long long* keys, long long n, int32_t* row, int32_t* len) {
    const long long k = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    row[k] = static_cast<int32_t>(keys[k] >> 32);
    len[k] = static_cast<int32_t>(keys[k] & 0xffffffffull);
}

// What the last profile of this thread left in the workspace ("prof.*" buffers).
struct ProfResult {
    bool valid = false;
    int R = 0;
    long long n_ins = 0, n_obs = 0;
    std::vector<int32_t> run_start, run_end;   // 1-based, inclusive
    std::string run_base;
};
static thread_local ProfResult g_prof;

// dense table + list -> distinct (row, length) pairs in ascending order with multiplicities, left in <tag>.row/.len/.mult
static int reduce_events(const std::string& tag, const PrEvents& e, long long rows, long long listed, long long* distinct, hipStream_t s) {
    *distinct = 0;
    const long long ncells = rows * PR_DENSE;
    unsigned long long* d_used;
    SL_TRY(scratch(tag + ".cells", 1, &d_used));
    unsigned long long cells = 0;
    if (ncells) {
        SL_HIP(hipMemsetAsync(d_used, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_pr_cells<false>, dim3(nblk(ncells, 256)), dim3(256), 0, s, e.dense, ncells, d_used, nullptr, nullptr);
        SL_HIP(hipGetLastError());
        SL_HIP(hipMemcpyAsync(&cells, d_used, sizeof cells, hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
    }
    const size_t total = static_cast<size_t>(cells) + static_cast<size_t>(listed);
    if (total == 0) return 0;
    unsigned long long *d_k0, *d_k1, *d_uk; long long *d_m0, *d_m1, *d_um, *d_nu;
    SL_TRY(scratch(tag + ".k0", total, &d_k0));
    SL_TRY(scratch(tag + ".k1", total, &d_k1));
    SL_TRY(scratch(tag + ".m0", total, &d_m0));
    SL_TRY(scratch(tag + ".m1", total, &d_m1));
    SL_TRY(scratch(tag + ".uk", total, &d_uk));
    SL_TRY(scratch(tag + ".mult", total, &d_um));
    SL_TRY(scratch(tag + ".nu", 1, &d_nu));
    if (cells) {
        SL_HIP(hipMemsetAsync(d_used, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_pr_cells<true>, dim3(nblk(ncells, 256)), dim3(256), 0, s, e.dense, ncells, d_used, d_k0, d_m0);
        SL_HIP(hipGetLastError());
    }
    if (listed) {
        SL_HIP(hipMemcpyAsync(d_k0 + cells, e.list, sizeof(unsigned long long) * static_cast<size_t>(listed), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_pr_ones, dim3(nblk(listed, 256)), dim3(256), 0, s, d_m0 + cells, listed);
        SL_HIP(hipGetLastError());
    }
    SL_TRY(radix_sort_pairs(tag + ".sorttmp", d_k0, d_k1, d_m0, d_m1, total, 32 + ceil_log2(static_cast<unsigned long long>(std::max<long long>(rows, 1))), s));
    size_t tmp = 0;
    SL_HIP(rocprim::reduce_by_key(nullptr, tmp, d_k1, d_m1, total, d_uk, d_um, d_nu, rocprim::plus<long long>(), rocprim::equal_to<unsigned long long>(), s));
    void* d_tmp;
    SL_TRY(ctx().buffer((tag + ".rbktmp").c_str(), tmp ? tmp : 16, &d_tmp));
    SL_HIP(rocprim::reduce_by_key(d_tmp, tmp, d_k1, d_m1, total, d_uk, d_um, d_nu, rocprim::plus<long long>(), rocprim::equal_to<unsigned long long>(), s));
    long long nu = 0;
    SL_HIP(hipMemcpyAsync(&nu, d_nu, sizeof nu, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    int32_t *d_row, *d_len;
    SL_TRY(scratch(tag + ".row", static_cast<size_t>(nu), &d_row));
    SL_TRY(scratch(tag + ".len", static_cast<size_t>(nu), &d_len));
    hipLaunchKernelGGL(k_pr_split, dim3(nblk(nu, 256)), dim3(256), 0, s, d_uk, nu, d_row, d_len);
    SL_HIP(hipGetLastError());
    *distinct = nu;
    return 0;
}

// The runs of the reference: maximal stretches of two or more equal characters.
static void reference_runs(const char* ref, int R, ProfResult* pr, std::vector<int32_t>* run_of) {
    pr->run_start.clear(); pr->run_end.clear(); pr->run_base.clear();
    run_of->assign(static_cast<size_t>(std::max(R, 1)), -1);
    for (int a = 0; a < R;) {
        int b = a + 1;
        while (b < R && ref[b] == ref[a]) ++b;
        if (b - a > 1) {
            (*run_of)[a] = static_cast<int32_t>(pr->run_start.size());
            pr->run_start.push_back(a + 1); pr->run_end.push_back(b); pr->run_base.push_back(ref[a]);
        }
        a = b;
    }
}

// h_off: the host copy of d_off (same values).  Scores and edit distances go to d_scores / d_edits (NULL: nowhere).
static int profile_impl(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const int64_t* h_off, int64_t n, int32_t max_len,
                        const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext, const char* ref, int R,
                        double* d_scores, int32_t* d_edits, int64_t* n_ins, int64_t* n_hp_runs, int64_t* n_hp_obs, hipStream_t s) {
    Context& c = ctx();
    g_prof.valid = false;
    if (R < 0) return fail("sarlacc_amd: negative reference length");
    if (n > std::numeric_limits<int>::max() - 8) return fail("sarlacc_amd: more than 2^31 reads in one call");
    for (const char* st : {"profile_align", "profile_kernel", "profile_reduce"}) c.stage_reset(st);
    std::vector<int32_t> run_of;
    reference_runs(ref, R, &g_prof, &run_of);
    const long long nruns = static_cast<long long>(g_prof.run_start.size());
    const int64_t total = n ? h_off[n] - h_off[0] : 0;

    PrArgs a{};
    a.R = R; a.nruns = static_cast<int>(nruns);
    int32_t* d_run_of;
    SL_TRY(upload("prof.run_of", run_of.data(), run_of.size(), &d_run_of, s));
    a.run_of = d_run_of;
    const size_t ncounts = 5 * static_cast<size_t>(R);
    SL_TRY(scratch("prof.counts", ncounts, &a.counts));
    SL_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * std::max<size_t>(ncounts, 1), s));
    // a read of L bases holds at most L / 64 insertions of 64 bases or more; a read base lies in the extended range of at
    // most two reference runs, so at most 2 L / 64 observations reach that length
    a.ins.cap = total / PR_DENSE + 1; a.obs.cap = total / (PR_DENSE / 2) + 1;
    const size_t ins_cells = (static_cast<size_t>(R) + 1) * PR_DENSE, obs_cells = static_cast<size_t>(nruns) * PR_DENSE;
    SL_TRY(scratch("prof.ins.dense", ins_cells, &a.ins.dense));
    SL_TRY(scratch("prof.obs.dense", obs_cells, &a.obs.dense));
    SL_TRY(scratch("prof.ins.list", static_cast<size_t>(a.ins.cap), &a.ins.list));
    SL_TRY(scratch("prof.obs.list", static_cast<size_t>(a.obs.cap), &a.obs.list));
    SL_HIP(hipMemsetAsync(a.ins.dense, 0, sizeof(int) * ins_cells, s));
    SL_HIP(hipMemsetAsync(a.obs.dense, 0, sizeof(int) * std::max<size_t>(obs_cells, 1), s));
    // [0] ins.used, [1] obs.used, [2] first_bad, [3] trouble
    unsigned long long* d_state;
    const unsigned long long state0[4] = {0, 0, ~0ull, 0};
    SL_TRY(upload("prof.state", state0, 4, &d_state, s));
    SL_HIP(hipStreamSynchronize(s));   // (state0 and run_of are this frame's)
    a.ins.used = d_state; a.obs.used = d_state + 1; a.first_bad = d_state + 2; a.trouble = reinterpret_cast<int*>(d_state + 3);

    // ---- chunks of reads: the aligner's two string buffers hold bytes + reads * R each
    const int64_t budget = static_cast<int64_t>(2) << 30;   // per buffer
    const int forced = option(OPT_PROFILE_CHUNK_READS);
    std::vector<int64_t> bounds{0};
    while (bounds.back() < n) {
        const int64_t lo = bounds.back();
        int64_t hi = lo + 1;
        if (forced > 0) hi = std::min<int64_t>(n, lo + forced);
        else while (hi < n && (h_off[hi + 1] - h_off[lo]) + (hi + 1 - lo) * static_cast<int64_t>(R) <= budget) ++hi;
        bounds.push_back(hi);
    }
    const int64_t nchunks = static_cast<int64_t>(bounds.size()) - 1;
    size_t slot_bytes = 1, chunk_reads = 1;
    for (int64_t k = 0; k < nchunks; ++k) {
        slot_bytes = std::max(slot_bytes, static_cast<size_t>((h_off[bounds[k + 1]] - h_off[bounds[k]]) + (bounds[k + 1] - bounds[k]) * static_cast<int64_t>(R)));
        chunk_reads = std::max(chunk_reads, static_cast<size_t>(bounds[k + 1] - bounds[k]));
    }
    uint8_t *d_aref, *d_aqry; int32_t* d_alen;
    SL_TRY(scratch("out.aref", slot_bytes, &d_aref));
    SL_TRY(scratch("out.aqry", slot_bytes, &d_aqry));
    SL_TRY(scratch("out.alen", chunk_reads, &d_alen));
    if (!d_scores) SL_TRY(scratch("prof.scores", static_cast<size_t>(std::max<int64_t>(n, 1)), &d_scores));
    if (!d_edits) SL_TRY(scratch("prof.edits", static_cast<size_t>(std::max<int64_t>(n, 1)), &d_edits));

    int bad_qual = std::numeric_limits<int>::max();
    unsigned long long first_bad = ~0ull;
    int bad_char = 0;
    for (int64_t k = 0; k < nchunks; ++k) {
        const int64_t lo = bounds[k], hi = bounds[k + 1];
        AlignJob job{{d_seq, d_qual, d_off + lo, hi - lo, max_len}, {enc_errors, enc_names, enc_n, gapopen, gapext}, ref, R, false, 2};
        job.stream = s;
        // the aligner addresses a slot by the read's offset in the whole batch: hand it the buffers shifted by the chunk's first offset
        job.out.d_scores = d_scores + lo; job.out.d_edits = d_edits + lo; job.out.d_aln_len = d_alen;
        job.out.d_aln_ref = d_aref - h_off[lo]; job.out.d_aln_qry = d_aqry - h_off[lo];
        ChunkOpts co;
        co.read_base = static_cast<int>(lo); co.init_bad = (k == 0); co.finish = true; co.stage = "profile_align";
        SL_TRY(run_align(job, &bad_qual, co));
        if (first_bad != ~0ull) continue;   // (the chain fails at that character; later chunks only matter for the aligner's own errors)
        a.aln_ref = d_aref; a.aln_qry = d_aqry; a.aln_len = d_alen; a.off = d_off + lo; a.n = hi - lo; a.read_base = lo;
        const unsigned gx = static_cast<unsigned>(std::max<long long>(1, std::min<long long>((hi - lo + PR_WAVES - 1) / PR_WAVES, static_cast<long long>(c.num_cu) * 4)));
        const unsigned gy = static_cast<unsigned>(std::max(1, (R + PR_TILE - 1) / PR_TILE));
        SL_TRY(c.stage_begin("profile_kernel", s));
        hipLaunchKernelGGL(k_profile_pairs, dim3(gx, gy), dim3(64 * PR_WAVES), 0, s, a);
        SL_HIP(hipGetLastError());
        SL_TRY(c.stage_end("profile_kernel", s));
        SL_HIP(hipMemcpyAsync(&first_bad, a.first_bad, sizeof first_bad, hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        if (first_bad != ~0ull) {   // the character itself, while its slot is still there
            const int64_t i = static_cast<int64_t>(first_bad >> 32) - lo, x = static_cast<int64_t>(first_bad & 0xffffffffull);
            int32_t m = 0;
            SL_HIP(hipMemcpy(&m, d_alen + i, sizeof m, hipMemcpyDeviceToHost));
            uint8_t ch = 0;
            SL_HIP(hipMemcpy(&ch, d_aqry + (h_off[lo + i] - h_off[lo]) + i * static_cast<int64_t>(R) + (m - 1 - x), 1, hipMemcpyDeviceToHost));
            bad_char = ch;
        }
    }
    c.counts["profile_chunks"] = static_cast<double>(nchunks);
    // errors in the chain's order: the aligner's first, then the profile's
    SL_TRY(first_error(n, h_off, nullptr, ref, R, bad_qual));
    if (first_bad != ~0ull) return fail("unknown character '%c' in alignment string", bad_char);
    unsigned long long state[4];
    SL_HIP(hipMemcpy(state, d_state, sizeof state, hipMemcpyDeviceToHost));
    const int trouble = static_cast<int>(state[3] & 0xffffffffull);
    if (trouble == 2) return fail("sarlacc_amd: internal error: an alignment does not spell its reference");
    if (trouble) return fail("sarlacc_amd: internal error: the list of long profile events overflowed");

    SL_TRY(c.stage_begin("profile_reduce", s));
    long long di = 0, dob = 0;
    SL_TRY(reduce_events("prof.ins", a.ins, static_cast<long long>(R) + 1, static_cast<long long>(state[0]), &di, s));
    SL_TRY(reduce_events("prof.obs", a.obs, nruns, static_cast<long long>(state[1]), &dob, s));
    SL_TRY(c.stage_end("profile_reduce", s));
    SL_HIP(hipStreamSynchronize(s));
    g_prof.R = R; g_prof.n_ins = di; g_prof.n_obs = dob; g_prof.valid = true;
    *n_ins = di; *n_hp_runs = nruns; *n_hp_obs = dob;
    return 0;
}

}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_profile_reads(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n, int32_t max_len,
                              const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                              const char* reference, int reference_len, double* d_scores, int32_t* d_edits, int64_t* n_ins,
                              int64_t* n_hp_runs, int64_t* n_hp_obs, void* stream) {
    SL_TRY(check_encoding(enc_errors, enc_names, enc_n));
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<int64_t> h_off(static_cast<size_t>(n) + 1, 0);
    if (n) {
        SL_HIP(hipMemcpyAsync(h_off.data(), d_off, sizeof(int64_t) * h_off.size(), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
    }
    return profile_impl(d_seq, d_qual, d_off, h_off.data(), n, max_len, enc_errors, enc_names, enc_n, gapopen, gapext, reference, reference_len,
                        d_scores, d_edits, n_ins, n_hp_runs, n_hp_obs, s);
}

int sarlacc_profile_reads(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                          const char* reference, int reference_len, double* scores, int32_t* edits, int64_t* n_ins,
                          int64_t* n_hp_runs, int64_t* n_hp_obs) {
    SL_TRY(check_encoding(enc_errors, enc_names, enc_n));
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    HostBatch hb;
    SL_TRY(upload_batch(seq, seq_off, qual, qual_off, n, &hb, s));
    if (hb.len_bad >= 0) {
        g_prof.valid = false;
        return first_error(n, seq_off, qual_off, reference, reference_len, std::numeric_limits<int>::max());
    }
    std::vector<int64_t> rel(static_cast<size_t>(n) + 1, 0);
    for (int64_t i = 0; i <= n && n; ++i) rel[i] = seq_off[i] - seq_off[0];
    double* d_scores; int32_t* d_edits;
    SL_TRY(scratch("out.scores", static_cast<size_t>(std::max<int64_t>(n, 1)), &d_scores));
    SL_TRY(scratch("out.edits", static_cast<size_t>(std::max<int64_t>(n, 1)), &d_edits));
    SL_TRY(profile_impl(hb.d_seq, hb.d_qual, hb.d_off, rel.data(), n, hb.max_len, enc_errors, enc_names, enc_n, gapopen, gapext, reference,
                        reference_len, d_scores, d_edits, n_ins, n_hp_runs, n_hp_obs, s));
    if (n && scores) SL_HIP(hipMemcpy(scores, d_scores, sizeof(double) * static_cast<size_t>(n), hipMemcpyDeviceToHost));
    if (n && edits) SL_HIP(hipMemcpy(edits, d_edits, sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyDeviceToHost));
    return 0;
}

int sarlacc_profile_fetch(int32_t* counts, int32_t* ins_pos, int32_t* ins_len, int64_t* ins_mult, int64_t cap_ins,
                          int32_t* run_start, int32_t* run_end, char* run_base, int64_t cap_runs,
                          int32_t* obs_run, int32_t* obs_len, int64_t* obs_mult, int64_t cap_obs) {
    const ProfResult& p = g_prof;
    if (!p.valid) return fail("sarlacc_amd: no profile to fetch (a successful sarlacc_*profile_reads must come first on this thread)");
    const long long nruns = static_cast<long long>(p.run_start.size());
    if (cap_ins < p.n_ins) return fail("sarlacc_amd: insertion buffers too small (%lld needed)", p.n_ins);
    if (cap_runs < nruns) return fail("sarlacc_amd: homopolymer run buffers too small (%lld needed)", nruns);
    if (cap_obs < p.n_obs) return fail("sarlacc_amd: homopolymer observation buffers too small (%lld needed)", p.n_obs);
    // the buffers of the last profile, by name; gone if the workspace was released in between
    auto held = [&](const char* name, size_t bytes, void** ptr) -> int {
        auto it = ctx().ws.find(name);
        if (it == ctx().ws.end() || !it->second.ptr || it->second.cap < bytes)
            return fail("sarlacc_amd: the results of the last profile are gone (workspace released)");
        *ptr = it->second.ptr;
        return 0;
    };
    struct Copy { const char* name; void* host; size_t bytes; };
    const size_t ni = static_cast<size_t>(p.n_ins), no = static_cast<size_t>(p.n_obs);
    const Copy copies[] = {{"prof.counts", counts, sizeof(int32_t) * 5 * static_cast<size_t>(p.R)},
                           {"prof.ins.row", ins_pos, sizeof(int32_t) * ni}, {"prof.ins.len", ins_len, sizeof(int32_t) * ni}, {"prof.ins.mult", ins_mult, sizeof(int64_t) * ni},
                           {"prof.obs.row", obs_run, sizeof(int32_t) * no}, {"prof.obs.len", obs_len, sizeof(int32_t) * no}, {"prof.obs.mult", obs_mult, sizeof(int64_t) * no}};
    void* src[7];
    for (int k = 0; k < 7; ++k) {
        if (copies[k].bytes == 0) continue;
        if (!copies[k].host) return fail("sarlacc_amd: null result buffer");
        SL_TRY(held(copies[k].name, copies[k].bytes, &src[k]));
    }
    if (nruns && (!run_start || !run_end || !run_base)) return fail("sarlacc_amd: null result buffer");
    for (int k = 0; k < 7; ++k)
        if (copies[k].bytes) SL_HIP(hipMemcpy(copies[k].host, src[k], copies[k].bytes, hipMemcpyDeviceToHost));
    for (long long r = 0; r < nruns; ++r) { run_start[r] = p.run_start[r]; run_end[r] = p.run_end[r]; run_base[r] = p.run_base[r]; }
    return 0;
}
}
