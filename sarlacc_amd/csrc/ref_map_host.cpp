// ref_map_host.cpp -- host side of ref_map.hip: argument checks, scratch, the rocPRIM sorts and scans between the
// launches, results, errors and the two C entry points (include/sarlacc_amd.h "resident reads assigned to references").
//
// Stage timers (sarlacc_stage_ms): refmap_candidates, and inside it refmap_entries_sort, refmap_probe, refmap_hits_sort,
// refmap_select; refmap_assign.  Counters (sarlacc_stage_count): refmap_hits, set by sarlacc_dev_sketch_candidates;
// refmap_checked and refmap_second_strand, set by sarlacc_dev_candidates_assign.
#include "ref_map.hpp"

#include "devprim.hpp"
#include "links_verify_core.hpp"

#include "../../include/sarlacc_amd.h"

namespace sarlacc {
namespace {

int state_begin(RmState** d_state, hipStream_t s) {
    SL_TRY(scratch("rm.state", 1, d_state));
    return rm_state_reset(*d_state, s);
}

int state_fetch(const RmState* d_state, RmState* host, hipStream_t s) {
    SL_HIP(hipMemcpyAsync(host, d_state, sizeof(RmState), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

int entry_refused(const char* side, unsigned long long e, int lb) {
    return fail("%s sketch %lld, bucket %lld: the entry is neither empty nor a hash of that bucket", side,
                static_cast<long long>(e >> lb) + 1, static_cast<long long>(e & ((1ull << lb) - 1)));
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_sketch_candidates(const uint64_t* d_ref_sketch, int64_t n_refs, const uint64_t* d_read_sketch, int64_t n_reads,
                                  int buckets, int min_shared, int max_candidates, int32_t* d_cand_ref, int32_t* d_cand_shared,
                                  int32_t* d_ncand, int64_t* n_hits, void* stream) {
    SL_TRY(count_ok(n_refs, "references"));
    SL_TRY(count_ok(n_reads, "reads"));
    const int lb = buckets_log2(buckets);
    if (lb < 0) return fail("sarlacc_amd: 'buckets' is a power of two in 16 .. 256");
    if (min_shared < 1 || min_shared > buckets) return fail("sarlacc_amd: 'min_shared' lies in 1 .. buckets");
    if (max_candidates < 1 || max_candidates > RM_MAX_CANDIDATES) return fail("sarlacc_amd: 'max_candidates' lies in 1 .. %d", RM_MAX_CANDIDATES);
    const long long mf = static_cast<long long>(n_refs) << lb, mr = static_cast<long long>(n_reads) << lb;
    if (mf >= SK_LIMIT) return fail("sarlacc_amd: %lld sketch entries (references x buckets): at most 2^31 - 1 in a call", mf);
    if (mr >= SK_LIMIT) return fail("sarlacc_amd: %lld sketch entries (reads x buckets): at most 2^31 - 1 in a call", mr);
    if (n_hits) *n_hits = 0;
    Context& c = ctx();
    c.counts["refmap_hits"] = 0;
    for (const char* name : {"refmap_candidates", "refmap_entries_sort", "refmap_probe", "refmap_hits_sort", "refmap_select"}) c.stage_reset(name);
    if (n_reads == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bits = ceil_log2(static_cast<unsigned long long>(n_refs));
    long long t = 0;
    const int rc = staged("refmap_candidates", s, [&]() -> int {
        if (n_refs == 0) return launch_rm_select(nullptr, nullptr, n_reads, lb, bits, min_shared, max_candidates, d_cand_ref, d_cand_shared, d_ncand, s);
        const size_t nf = static_cast<size_t>(mf), nr = static_cast<size_t>(mr);
        RmState* d_state;
        uint64_t* d_hash;
        int32_t *d_ref, *d_sref, *d_dir, *d_first, *d_count;
        int64_t* d_begin;
        SL_TRY(state_begin(&d_state, s));
        SL_TRY(scratch("rm.hash", nf, &d_hash));
        SL_TRY(scratch("rm.ref", nf, &d_ref));
        SL_TRY(scratch("rm.sref", nf, &d_sref));
        SL_TRY(scratch("rm.dir", static_cast<size_t>(buckets) + 1, &d_dir));
        SL_TRY(scratch("rm.first", nr, &d_first));
        SL_TRY(scratch("rm.count", nr + 1, &d_count));
        SL_TRY(scratch("rm.begin", nr + 1, &d_begin));
        SL_TRY(staged("refmap_entries_sort", s, [&]() -> int {
            SL_TRY(launch_rm_ref_entries(d_ref_sketch, mf, lb, d_ref, d_state, s));
            // stable: entries of equal hash stay in reference order; the empty ones sort behind every hash
            return radix_sort_pairs("rm.sort", const_cast<uint64_t*>(d_ref_sketch), d_hash, d_ref, d_sref, nf, 64, s);
        }));
        RmState st;
        uint64_t *d_pair = nullptr, *d_spair = nullptr;
        SL_TRY(staged("refmap_probe", s, [&]() -> int {
            SL_TRY(launch_rm_directory(d_hash, mf, lb, d_dir, s));
            SL_TRY(launch_rm_probe_count(d_read_sketch, mr, lb, d_hash, d_dir, d_first, d_count, d_state, s));
            SL_TRY(exclusive_scan("rm.scan", d_count, d_begin, nr + 1, s));
            SL_HIP(hipMemcpyAsync(&t, d_begin + mr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            SL_TRY(state_fetch(d_state, &st, s));
            // nothing that rests on a refused entry is launched
            if (st.bad_ref_entry != ~0ull || st.bad_read_entry != ~0ull || t == 0 || t >= SK_LIMIT) return 0;
            SL_TRY(scratch("rm.pair", static_cast<size_t>(t), &d_pair));
            SL_TRY(scratch("rm.spair", static_cast<size_t>(t), &d_spair));
            return launch_rm_probe_fill(d_first, d_begin, d_sref, mr, lb, bits, d_pair, s);
        }));
        if (st.bad_ref_entry != ~0ull) return entry_refused("reference", st.bad_ref_entry, lb);
        if (st.bad_read_entry != ~0ull) return entry_refused("read", st.bad_read_entry, lb);
        if (t >= SK_LIMIT) return fail("sarlacc_amd: %lld hits of read sketches in reference sketches: at most 2^31 - 1 in a call", t);
        if (t > 0) {
            const int key_bits = bits + ceil_log2(static_cast<unsigned long long>(n_reads));
            SL_TRY(staged("refmap_hits_sort", s, [&] { return radix_sort_keys("rm.sort", d_pair, d_spair, static_cast<size_t>(t), key_bits, s); }));
        }
        return staged("refmap_select", s, [&] {
            return launch_rm_select(d_spair, d_begin, n_reads, lb, bits, min_shared, max_candidates, d_cand_ref, d_cand_shared, d_ncand, s);
        });
    });
    SL_TRY(rc);
    SL_HIP(hipStreamSynchronize(s));
    c.counts["refmap_hits"] = static_cast<double>(t);
    if (n_hits) *n_hits = t;
    return 0;
}

int sarlacc_dev_candidates_assign(const uint8_t* d_ref_seq, const int64_t* d_ref_off, int64_t n_refs, const uint8_t* d_read_seq,
                                  const int64_t* d_read_off, int64_t n_reads, const int32_t* d_cand_ref, const int32_t* d_cand_shared,
                                  int max_candidates, int bandwidth, int64_t max_diff_ppm, int both_strands, int32_t* d_reference,
                                  uint8_t* d_strand, int32_t* d_dist, int32_t* d_shared, int32_t* d_cand_dist, uint8_t* d_cand_strand,
                                  int64_t* n_checked, void* stream) {
    SL_TRY(count_ok(n_refs, "references"));
    SL_TRY(count_ok(n_reads, "reads"));
    if (max_candidates < 1 || max_candidates > RM_MAX_CANDIDATES) return fail("sarlacc_amd: 'max_candidates' lies in 1 .. %d", RM_MAX_CANDIDATES);
    if (bandwidth < 0 || bandwidth > LV_MAX_BANDWIDTH) return fail("sarlacc_amd: 'bandwidth' lies in 0 .. %d", LV_MAX_BANDWIDTH);
    if (max_diff_ppm >= LV_PPM) return fail("sarlacc_amd: 'max_diff_ppm' lies in 0 .. 999999, or is negative: no check");
    if (n_checked) *n_checked = 0;
    Context& c = ctx();
    c.counts["refmap_checked"] = 0;
    c.counts["refmap_second_strand"] = 0;
    c.stage_reset("refmap_assign");
    if (n_reads == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool check = max_diff_ppm >= 0;
    const size_t slots = static_cast<size_t>(n_reads) * max_candidates;
    RmState* d_state;
    SL_TRY(state_begin(&d_state, s));
    if (check && !d_cand_dist) SL_TRY(scratch("rm.cand_dist", slots, &d_cand_dist));
    if (check && !d_cand_strand) SL_TRY(scratch("rm.cand_strand", slots, &d_cand_strand));
    const AssignArgs a{d_ref_seq, d_ref_off, n_refs, d_read_seq, d_read_off, n_reads, d_cand_ref, max_candidates, bandwidth,
                       max_diff_ppm, both_strands ? 1 : 0};
    RmState st;
    // the stage in two segments: nothing that rests on a refused candidate, reference or read is launched
    if (check) {
        SL_TRY(c.stage_begin("refmap_assign", s));
        SL_TRY(launch_rm_assign(a, d_cand_dist, d_cand_strand, d_state, s));
        SL_TRY(c.stage_end("refmap_assign", s));
        SL_TRY(state_fetch(d_state, &st, s));
        if (st.bad_cand != ~0ull) return fail("read %lld: candidate outside 0 .. n_refs - 1", static_cast<long long>(st.bad_cand) + 1);
        if (st.bad_ref != ~0ull)
            return fail("reference %lld: its offsets do not ascend inside the sequence buffer, or it has 2^31 bases or more", static_cast<long long>(st.bad_ref) + 1);
        if (st.bad_read != ~0ull)
            return fail("read %lld: its offsets do not ascend inside the sequence buffer, or it has 2^31 bases or more", static_cast<long long>(st.bad_read) + 1);
    }
    SL_TRY(c.stage_begin("refmap_assign", s));
    SL_TRY(launch_rm_choose(a, check ? 1 : 0, d_cand_shared, d_cand_dist, d_cand_strand, d_reference, d_strand, d_dist, d_shared, d_state, s));
    SL_TRY(c.stage_end("refmap_assign", s));
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_cand != ~0ull) return fail("read %lld: candidate outside 0 .. n_refs - 1", static_cast<long long>(st.bad_cand) + 1);
    c.counts["refmap_checked"] = static_cast<double>(st.n_checked);
    c.counts["refmap_second_strand"] = static_cast<double>(st.n_second);
    if (n_checked) *n_checked = static_cast<int64_t>(st.n_checked);
    return 0;
}
}
