// consensus.hpp -- what consensus.hip (the vote kernels and the two functions that launch them) and consensus_host.cpp
// (route plan, tables, row tables, scratch, results and errors, the host-libm fix-up, the C entry points) share.  The
// kernels read ConsArgs and the constants below as they stand.
#pragma once

#include "msa_common.hpp"

#include <cmath>

namespace sarlacc {

struct ConsArgs {
    const uint8_t* aln;
    const int64_t* aln_off;    // per row
    const int64_t* grp_rows;   // [ngroups+1]
    long long ngroups;
    const uint8_t* qual;       // quality mode only
    const int64_t* qual_off;   // per row (same row numbering as aln), or per read when row_read is set
    const int32_t* row_read;   // optional: 1-based read id of every row (qualities stay in read order)
    const double* right;       // [navail] log1p(-e)
    const double* wrong;       // [navail] log(e/3)
    const double* vec;         // k_consensus_q4: [(5 * navail + 1)][4] per-(read character, quality) additions to the A,C,G,T scores
    int qoffset, navail, max_rows;
    double mincov, pseudo, ln10;
    const int64_t* out_off;    // [ngroups] start of the group's output (= offset of its first row)
    uint8_t* cons;
    uint8_t* phred;
    double* lerr;              // optional
    int32_t* cons_len;         // [ngroups]
    int8_t* row_status;        // quality: 0 ok, 1 bad quality char, 2 shorter, 3 longer
    unsigned long long* first_bad_char;  // basic: min byte index of an unknown character
    // near-boundary columns to be resolved on the host
    int* fix_count;
    int fix_cap;
    long long* fix_pos;        // output byte index
    double* fix_val;           // 4 per entry: sorted scores (quality) or {max,total,0,0} (basic)
    int* fix_grp;              // k_consensus_qf: group of the entry (entries of groups handed to the generic kernel are void)
    // k_consensus_qf (fast path) and its hand-over to k_consensus_q4
    const double* strip;       // [(navail + 1)][QF_STRIP][QF_SLOTS]: per quality the strip (w w w r w w w), replicated; last row zeros
    int* gflag;                // per group: 1 = the fast kernel met something it does not handle; the generic kernel redoes the group
    int only_flagged;          // k_consensus_q4: skip groups whose flag is 0
    long long aln_bytes, qual_bytes;   // sizes of the two buffers (the fast kernel reads whole dwords)
    // k_consensus_code: the rows as 16-bit vote codes written by the MSA stage (CodeSpec, common.hpp)
    const uint16_t* codes;     // same offsets as aln, in cells
    const double* strip8;      // [(navail + 1)][CODE_STRIP][QF_SLOTS]: (w w w r w w w w) per quality, zero row last
    int* code_bad;             // smallest row with a quality below the encoding (INT_MAX: none)
};

__host__ __device__ __forceinline__ double r_log1pexp(double x) {
    // R nmath log1pexp: x <= 18 -> log1p(exp x); 18 < x <= 33.3 -> x + exp(-x); else x
    if (x <= 18.) return log1p(exp(x));
    if (x > 33.3) return x;
    return x + exp(-x);
}

// The reference's log error of a column from its four scores in ascending order: a running log-sum-exp, less the
// largest score.  Host and device compile the same source, each against its own libm.
__host__ __device__ __forceinline__ double log_error(double a, double b, double c, double d) {
    double denom = a;
    denom += r_log1pexp(b - denom);
    denom += r_log1pexp(c - denom);
    const double err3 = denom;
    denom += r_log1pexp(d - denom);
    return err3 - denom;
}

constexpr int Q4_RB = 5;   // k_consensus_q4: rows fetched per batch

// k_consensus_qf: the LDS table holds, per quality value, the strip (w w w r w w w), every double replicated for 16 lane slots
constexpr int QF_SLOTS = 16;
constexpr int QF_STRIP = 7;
constexpr int QF_ROWB = QF_STRIP * QF_SLOTS * 8;   // 896 bytes per quality value
constexpr int QF_RB = 6;                           // rows per batch: two scans of three packed counts
constexpr int QF_THREADS = 1024;

// k_consensus_code: the strip of CODE_STRIP doubles (msa_common.hpp)
constexpr int QC_RB = 5;
constexpr int QC_ROWB = CODE_STRIP * QF_SLOTS * 8;   // 1024 bytes per quality value

// ---- which kernels a call runs ----
// BASIC / GENERIC: k_consensus<false> / k_consensus<true> (one column per lane; the only kernel that returns log errors and
// the only one for alignments too deep for k_consensus_q4's LDS); Q4: k_consensus_q4 alone; QF_Q4: k_consensus_qf, then
// k_consensus_q4 on the groups it flagged; CODE: k_consensus_code on the vote codes of the MSA stage.
// (sarlacc_stage_count "consensus_route" reports the value.)
enum ConsRoute { CONS_BASIC = 0, CONS_GENERIC = 1, CONS_Q4 = 2, CONS_QF_Q4 = 3, CONS_CODE = 4 };

struct ConsLaunch {
    size_t lds = 0;           // dynamic LDS bytes
    unsigned grid = 0, block = 0;
    bool raise_lds = false;   // lift the kernel's dynamic-LDS limit to `lds` before the launch
};
// A call's launches, by the kernel each belongs to: launch_vote takes the kernel from the route and everything else from here.
struct ConsPlan {
    ConsRoute route = CONS_BASIC;
    ConsLaunch vote;          // the route's kernel: k_consensus<QUALITY>, k_consensus_q4 or k_consensus_code
    ConsLaunch qf;            // k_consensus_qf ahead of it (CONS_QF_Q4 only)
    bool refused = false;     // an alignment has more rows than the one-column kernel's LDS holds: nothing is launched
};

// ---- consensus.hip ----
// The vote of a call on stream s (run again as it is when the boundary list was too short).  CONS_QF_Q4 is two launches,
// the second with only_flagged = 1.
int launch_vote(const ConsPlan& plan, const ConsArgs& a, hipStream_t s);
// Kept columns of a's groups (a.cons / a.phred / a.lerr at a.out_off, a.cons_len of them) to d_cons / d_phred / d_lerr at d_dst[g].
int launch_compact(const ConsArgs& a, const long long* d_dst, uint8_t* d_cons, uint8_t* d_phred, double* d_lerr, hipStream_t s);

}  // namespace sarlacc
