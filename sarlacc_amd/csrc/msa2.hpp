// msa2.hpp -- what msa2.hip (the spec v2 kernels and the functions that launch them: the device half of a batch) and
// msa2_host.cpp (batch plan, memory budget and the cut into pipelined batches, the row buffer, the scoring domain, the split
// into spec v1 and spec v2 groups, the work counters: msa_run) share.  The tables below are read by the kernels as they stand.
#pragma once

#include "msa_common.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace sarlacc {

constexpr int M2_MAXN = 64;          // group sizes aligned by spec v2 (member sets are 64-bit masks; 32-bit ones in the kernels of groups of up to 32)
constexpr int M2_N32 = 32;
typedef unsigned long long m2_mask;
constexpr int M2_NB = 24;   // groups of up to M2_NB reads: one wavefront; up to 32: 8 wavefronts; 33 .. 64: M2_NWD (k_m2_group; sweeps: profiles/r03_exp_m2_class_thresholds_v1.txt, r04_exp_m2_classes_v1.txt -- a 4-wavefront class between the first two lost in every sweep and is gone)
constexpr int M2_CAP = 16;           // partner columns per row (spec v2, step 5)
// profile capacity of the first pass: same-molecule reads grow a profile by 10-20 %, one or two unrelated reads in
// the cluster by their length each
// ... by group size: a cluster of n reads out of umi_group holds about n / 10 molecules (UMI collisions), whose profiles do
// not align -- one more read length per 8 reads beyond 11.  (With 3 maxlen + 64 for every size the clusters of three and
// more molecules, the most expensive groups of a call, ran out of columns and were done twice, all-pairs alignments
// included: 85 ms of the 657 ms merge stage of bench.py's pipeline workload.)
static inline long long m2_fast_width(long long n, long long maxlen) {
    if (option(OPT_MSA2_TIGHT_PROFILES)) return 2 * maxlen + 64;
    return (3 + std::max(0LL, (n - 4) / 8)) * maxlen + 64;
}
// unit weights: the packed library records and the rows that go with them (k_m2_extend_unit, k_m2_group<true, ...>)
static inline bool m2_unit_weights(int ma, int mm) { return ma <= 1 && mm <= 1 && !option(OPT_MSA2_GENERAL_ROWS); }
static inline int m2_ext_planes(bool unitw) { return unitw ? 3 : 4; }

struct M2Member {         // one read of a group
    long long seq_off;    // into d_seq
    long long map_base;   // into d_map: (n - 1) arrays of `len` entries, the other members in member order
    long long col_base;   // into d_col
    long long ext_base;   // the group's (M2Group::ext_base): k_m2_extend works from the member table alone
    int len;
    int first_member;     // of its group
    int n;                // reads in its group
    int lmax;             // the group's longest read
};
struct M2Group {
    int first_member;     // member a of the group is members[first_member + a]; joins at first_member + k
    int n;
    int wcap;             // capacity of a profile in columns
    int lmax;             // the group's longest read: stride of the extended library's records per pair
    long long pos_base;   // into d_pos: n * wcap
    long long first_job;  // pairwise job of (a, b), a < b: first_job + a n - a (a + 1) / 2 + b - a - 1
    long long dist_base;  // into the tree kernel's scratch: n * n + n doubles
    long long ext_base;   // into a plane of the extended library: n (n - 1) / 2 pairs x lmax records
    long long map0, col0; // map_base / col_base of the group's first member
};

// counters of one call (sarlacc_stage_count): how often spec v2's own rules act, and the chain's fallback
enum { M2C_ROWS, M2C_ROWS_CAPPED, M2C_ENT_FILTERED, M2C_ROWS_FILTERED, M2C_ENT_KEPT, M2C_JOINS, M2C_JOINS_HBMQ,
       M2C_GATHERS,   // wave-wide gather instructions of the rows phase (positions, map entries, records, columns): a lower bound
       // where the wavefronts' time goes (s_memtime cycles summed over the wavefronts) and when they leave (s_memrealtime, 100 MHz)
       M2C_CYC_ROWS, M2C_CYC_CHAIN, M2C_CYC_WALK, M2C_CYC_RENUMBER, M2C_T_START, M2C_T_FIRST_EXIT, M2C_T_LAST_EXIT,
       M2C_T_EXIT1, M2C_T_EXIT4, M2C_T_EXIT8,   // last exit of the instantiations: one wavefront per group / groups of 33 .. 64 reads / 8 wavefronts
       M2C_N };
// ... and what the host counts beside them: the values of a call (msa2_core keeps both kinds in one array) and its seconds
// outside the kernels, by part (m2_host_time).  Their names: the table in msa2_host.cpp.
enum { M2H_PAIRS = M2C_N, M2H_CELLS, M2H_SECOND_PASS, M2H_BATCHES, M2H_VALUES,
       M2H_T_PLAN = M2H_VALUES, M2H_T_UPLOAD_ALLOC, M2H_T_PAIRWISE_LAUNCH, M2H_T_ROWS, M2H_T_TOTAL };

struct M2Args {
    const uint8_t* seq;
    const M2Group* groups;
    const M2Member* members;
    int ngroups;
    int ma, mm;
    const uint16_t* map;
    const int2* stats;
    double* dist;
    int2* joins;
    m2_mask* first;                // per member: the members it meets as part of the FIRST child (k_m2_first)
    uint32_t* ext;                 // the extended library (k_m2_extend): plane 0 here, planes 1 .. 2 (unit weights) or 1 .. 3 at
    long long ext_off1, ext_plane; //   ext + ext_off1 + (k - 1) ext_plane -- plane 0 may live in a buffer of its own (m2_merge)
    uint16_t* col;                 // (a column is < 65535: 16 bits halve the bytes of the walk's column gathers)
    uint16_t* pos;
    int* ovf;                      // per group: a profile outgrew its capacity
    int32_t* width;                // per group: columns of the final profile
    // ---- k_m2_group: the launch's range of groups [g0, g1), work counter, counters, per-workgroup scratch (w_rows columns each) ----
    int g0, g1;
    int* next;
    unsigned long long* counters;
    unsigned long long* w_ent;     // match list: (row << 48) | (column << 32) | weight; M2_CAP entries per column
    unsigned* w_pred;              // per match: 1 + index of its predecessor on its best chain (0: none)
    int* w_part;                   // partner column of column i of the first child, -1 if unmatched
    int* w_nca;                    // new numbers of the first child's columns
    int* w_ncb;                    // ... of the second child's
    int* w_pb;                     // partner row of column j of the second child
    unsigned long long* w_q;       // prefix maxima over all columns (the chain's fallback when the LDS ring cannot answer)
    long long w_rows;
    int chain_hbm;                 // testing: the prefix maxima in HBM from the start (what the LDS ring falls back to)
    // ---- row writer ----
    uint8_t* out;                  // gapped rows
    uint16_t* out16;               // rows as vote codes instead of characters (CodeSpec, common.hpp): out16 != nullptr
    const uint8_t* qual;           // laid out like seq
    int qoffset, navail;
    int* bad;
};

// One batch of groups (`ids`: indices into the caller's group list) through the v2 kernels.
// exact_w = false: fast profile capacity (3 maxlen + 64 columns); groups that outgrow it come back flagged.
// exact_w = true: profiles as wide as the sum of the read lengths, nothing can overflow.
// Leaves the batch's state (pos, members ...) in the "m2*" workspaces for the row writer.
struct M2Batch {
    std::vector<int64_t> ids;      // caller's group indices, by decreasing group size
    std::vector<size_t> slot;      // position of each in the caller's order (msa2_core)
    std::vector<M2Group> groups;
    std::vector<M2Member> members;
    std::vector<int> member_group;
    size_t njobs = 0;             // pairwise jobs of the batch (the table itself exists on the device only, k_m2_jobs)
    std::vector<int32_t> width;   // per group of the batch
    std::vector<int> ovf;
    M2Args a{};                   // device pointers
    int* d_member_group = nullptr;
    int max_len = 0, max_wcap = 0, max_n = 0;
    long long map_n = 0, col_n = 0, pos_n = 0;   // entries of the batch's maps, columns and positions (m2_plan)
    long long ext_n = 0;          // records per plane of the extended library
    bool alias_tiles = false;     // plane 0 of the library in the pairwise kernel's tile buffer (a call of one batch)
    MsaJobSummary jsum;           // band classes and cell count of `jobs`
    hipEvent_t pair_done = nullptr;   // the all-pairs alignments of the batch have finished (m2_prepare -> m2_merge)
};

// streams of the side-by-side instantiations of k_m2_group (created once per process and device, non-blocking: the
// caller's stream may be the legacy default one)
struct M2Streams {
    std::vector<hipStream_t> st;
    std::vector<hipEvent_t> join;
    hipEvent_t fork = nullptr;
    hipEvent_t pair[2] = {nullptr, nullptr};   // "alignments of the batch in workspace set k are done"
    int device = -1;
    int ensure(int n);
};
M2Streams& m2_streams();

double m2_now();
// host seconds of the MSA stage outside its kernels, by part (an M2H_T_* value; sarlacc_stage_count "msa_host_<part>_s")
void m2_host_time(int part, double t0);

// ---- the device half of a batch (msa2.hip) ----
// First half: tables to the device, workspaces, the all-pairs alignments -- on stream `s`, which runs ahead of the merging.
int m2_prepare(M2Batch& B, const std::string& pf, const uint8_t* d_seq, double match, double mismatch, double gap_extension,
               double gap_opening, int bandwidth, double* cells, bool first_of_call, hipStream_t s);
// Second half: guide trees, the extended library, all the merging, widths back to the host; counters[M2C_*] are added to.
int m2_merge(M2Batch& B, const std::string& pf, double* counters, hipStream_t s);
// rows of the batch's groups (except those sent to the next pass, whose width is 0) at out + off[group of the caller's list]
int m2_write_batch(M2Batch& B, const std::string& pf, const std::vector<long long>& off_of_batch_group, void* d_out,
                   const CodeSpec& code, hipStream_t s);
// msa_run's final gather: group g's nbytes[g] bytes from src1 (from1[g], spec v1's buffer) or src2 (spec v2's) at src_off[g]
// to d_final + dst_off[g]
int msa_rows_gather(const uint8_t* src1, const uint8_t* src2, const std::vector<long long>& src_off, const std::vector<long long>& dst_off,
                    const std::vector<long long>& nbytes, const std::vector<char>& from1, bool have1, uint8_t* d_final, hipStream_t s);

}  // namespace sarlacc
