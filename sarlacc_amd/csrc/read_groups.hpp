// read_groups.hpp -- what read_groups.hip (the kernels and the functions that launch them) and read_groups_host.cpp
// (argument checks, scratch, the rocPRIM sorts and scans between the launches, results and errors, the C entry points)
// share.
#pragma once

#include "common.hpp"

namespace sarlacc {

constexpr uint64_t RG_EMPTY = ~0ull;         // a free slot of the name table; a taken one holds tag << 32 | read index
constexpr uint64_t RG_UNMAPPED = 1ull << 63;   // the locus sort key of a read without a record: behind every mapped read
constexpr uint32_t RG_NO_LABEL = 0xffffffffu;  // the CSR sort key of a negative label: behind every group
constexpr int RG_MAX_REF = 1 << 30;          // seqname codes lie below this (the locus key keeps 30 bits of them)

// A flat string set in HBM: n names, n + 1 offsets.
struct NameSet {
    const uint8_t* chars;
    const int64_t* off;
    long long n;
};

// The words a call's kernels report through (one scratch block, set up by rg_state_reset): every `bad_*` and `dup` is an
// atomicMin over ~0, the counters are sums.
struct RgState {
    unsigned long long dup;             // rule 1: K << 32 | J, 0-based
    unsigned long long bad_read_off;    // lowest read whose offsets do not ascend inside the buffer
    unsigned long long bad_rec_off;     // ... record
    unsigned long long bad_value;       // lowest item with a value outside its domain (pick: record; locus: read)
    unsigned long long unmatched;       // records that name no read
    long long n_groups, n_members;
};

// ---- read_groups.hip ----
int rg_state_reset(RgState* d_state, hipStream_t s);
// key length and hash of every read name (cut at the first space or tab)
int launch_name_keys(NameSet reads, int hash_bits, int32_t* klen, uint64_t* hash, RgState* st, hipStream_t s);
// table: nslots (a power of two, >= 2 n) words, RG_EMPTY everywhere on entry
int launch_name_build(NameSet reads, const int32_t* klen, const uint64_t* hash, uint64_t* table, long long nslots, hipStream_t s);
int launch_name_check(NameSet reads, const int32_t* klen, const uint64_t* hash, const uint64_t* table, long long nslots,
                      RgState* st, hipStream_t s);
int launch_name_probe(NameSet reads, const int32_t* klen, const uint64_t* table, long long nslots, NameSet recs, int hash_bits,
                      int32_t* read_of_record, RgState* st, hipStream_t s);
// best: n_reads words, 0 on entry
int launch_pick(const int32_t* read_of_record, const int32_t* width, long long n_records, long long n_reads,
                unsigned long long* best, int32_t* record_of_read, int32_t* records_per_read, RgState* st, hipStream_t s);

struct LocusArgs {
    const int32_t* ref; const uint8_t* strand; const int32_t* start; const int32_t* width;
    const int32_t* record_of_read;
    long long n_records, n_reads, maxgap;
    int ignore_strand;
};
int launch_locus_keys(const LocusArgs& a, uint64_t* key, int32_t* idx, RgState* st, hipStream_t s);
int launch_locus_ends(const LocusArgs& a, const uint64_t* skey, const int32_t* sidx, uint32_t* seg, int64_t* end, hipStream_t s);
int launch_locus_flags(const LocusArgs& a, const uint64_t* skey, const uint32_t* seg, const int64_t* runmax, int32_t* flag, hipStream_t s);
int launch_locus_scatter(const LocusArgs& a, const uint64_t* skey, const int32_t* sidx, const int32_t* flag, const int32_t* before,
                         int32_t* label, RgState* st, hipStream_t s);

int launch_csr_keys(const int32_t* label, long long n, uint32_t* key, int32_t* member, hipStream_t s);
int launch_csr_heads(const uint32_t* skey, long long n, int32_t* head, hipStream_t s);
int launch_csr_offsets(const uint32_t* skey, long long n, const int32_t* head, const int32_t* before, int64_t* group_off,
                       RgState* st, hipStream_t s);

}  // namespace sarlacc
