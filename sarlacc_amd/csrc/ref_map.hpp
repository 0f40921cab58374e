// ref_map.hpp -- what ref_map.hip (the kernels and the functions that launch them) and ref_map_host.cpp (argument checks,
// scratch, the rocPRIM sorts and scans between the launches, results and errors, the two C entry points) share.
#pragma once

#include "sketch.hpp"

namespace sarlacc {

constexpr int RM_MAX_CANDIDATES = 16;

// The words a call's kernels report through (one scratch block, set up by rm_state_reset): every `bad_*` is an atomicMin
// over ~0, the counters are sums of ones (their value does not depend on the order of arrival).
struct RmState {
    unsigned long long bad_ref_entry;     // lowest entry of the reference sketches that lies outside its bucket
    unsigned long long bad_read_entry;    // the same of the read sketches
    unsigned long long bad_cand;          // lowest read with a candidate outside 0 .. n_refs - 1
    unsigned long long bad_ref;           // lowest reference whose offsets do not ascend inside the buffer
    unsigned long long bad_read;          // the same of the reads
    unsigned long long n_checked;         // candidates handed to the alignment check
    unsigned long long n_second;          // pairs whose reverse orientation was computed
};

// a launch of the check of rule M4: slot i = r * k + s holds candidate s of read r; w the bandwidth, 0 .. 127
struct AssignArgs {
    const uint8_t* ref_seq;
    const int64_t* ref_off;
    long long n_refs;
    const uint8_t* read_seq;
    const int64_t* read_off;
    long long n_reads;
    const int32_t* cand_ref;
    int k;
    int w;
    long long max_diff_ppm;
    int both_strands;
};

// ---- ref_map.hip ----
int rm_state_reset(RmState* d_state, hipStream_t s);
// ref[e] = e >> log2_buckets for the m = n_refs << log2_buckets entries; an entry that is neither empty nor inside
// bucket e mod buckets goes to st->bad_ref_entry
int launch_rm_ref_entries(const uint64_t* sketch, long long m, int log2_buckets, int32_t* ref, RmState* st, hipStream_t s);
// dir[j], j = 0 .. buckets: the first of the m sorted hashes that is not below j << (64 - log2_buckets); dir[buckets]
// is the first empty entry
int launch_rm_directory(const uint64_t* hash, long long m, int log2_buckets, int32_t* dir, hipStream_t s);
// Per entry e of the read sketches (mr of them; count has mr + 1 entries, count[mr] = 0): first[e] and count[e], the
// run of sorted reference entries that hold the entry's hash, looked for inside its bucket's segment alone.
int launch_rm_probe_count(const uint64_t* read_sketch, long long mr, int log2_buckets, const uint64_t* hash, const int32_t* dir,
                          int32_t* first, int32_t* count, RmState* st, hipStream_t s);
// pair[begin[e] + d] = read << bits | ref[first[e] + d] for d below what the count pass saw (begin: the mr + 1 scanned counts)
int launch_rm_probe_fill(const int32_t* first, const int64_t* begin, const int32_t* ref, long long mr, int log2_buckets, int bits,
                         uint64_t* pair, hipStream_t s);
// Over the pair keys in ascending order, read r's between begin[r << log2_buckets] and begin[(r + 1) << log2_buckets]
// (begin may be null: no hit at all): the runs of at least min_shared equal keys, ranked by length descending, then
// reference ascending; the first k of them to row r of cand_ref / cand_shared (unused slots -1 / 0), their number to ncand.
int launch_rm_select(const uint64_t* pair, const int64_t* begin, long long n_reads, int log2_buckets, int bits, int min_shared, int k,
                     int32_t* cand_ref, int32_t* cand_shared, int32_t* ncand, hipStream_t s);
// Rule M4 per slot (n_reads * k > 0 of them): cand_dist (-1: unused slot or fails), cand_strand; refusals and the two
// counters go to st.
int launch_rm_assign(const AssignArgs& a, int32_t* cand_dist, uint8_t* cand_strand, RmState* st, hipStream_t s);
// Rule M5 per read.  check != 0: the passing slot of smallest cand_dist, the lowest among equals.  check == 0: slot 0,
// with dist -1 and strand 0; cand_dist / cand_strand (may be null then) are set to -1 / 0 and the candidates' range is
// checked here.
int launch_rm_choose(const AssignArgs& a, int check, const int32_t* cand_shared, int32_t* cand_dist, uint8_t* cand_strand,
                     int32_t* reference, uint8_t* strand, int32_t* dist, int32_t* shared, RmState* st, hipStream_t s);

}  // namespace sarlacc
