// sketch_host.cpp -- host side of sketch.hip and links_verify.hip: argument checks, scratch, the rocPRIM sorts and scans
// between the launches, results, errors and the four C entry points (include/sarlacc_amd.h "reference-free pre-groups of
// a read batch").
//
// Stage timers (sarlacc_stage_ms): sketch_reads, sketch_entries_sort, sketch_pairs, sketch_pairs_sort, sketch_select,
// sketch_verify, components.  Counters (sarlacc_stage_count): components_rounds, sketch_verify_pairs (links looked at),
// sketch_verify_second_strand (pairs whose reverse orientation was computed); the two are 0 after sarlacc_dev_sketch_links.
#include "sketch.hpp"

#include "devprim.hpp"
#include "links_verify_core.hpp"

#include "../../include/sarlacc_amd.h"

namespace sarlacc {
namespace {

int state_begin(SkState** d_state, hipStream_t s) {
    SL_TRY(scratch("sk.state", 1, d_state));
    return sk_state_reset(*d_state, s);
}

int state_fetch(const SkState* d_state, SkState* host, hipStream_t s) {
    SL_HIP(hipMemcpyAsync(host, d_state, sizeof(SkState), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_sketch_reads(const uint8_t* d_seq, const int64_t* d_off, int64_t n, int k, int buckets, int canonical,
                             uint64_t* d_sketch, int32_t* d_nkmers, void* stream) {
    SL_TRY(count_ok(n, "reads"));
    if (k < 5 || k > 31) return fail("sarlacc_amd: 'k' lies in 5 .. 31");
    const int lb = buckets_log2(buckets);
    if (lb < 0) return fail("sarlacc_amd: 'buckets' is a power of two in 16 .. 256");
    if (n == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    SkState* d_state;
    SL_TRY(state_begin(&d_state, s));
    const SketchArgs a{d_seq, d_off, n, k, lb, canonical ? 1 : 0};
    SL_TRY(staged("sketch_reads", s, [&] { return launch_sketch(a, d_sketch, d_nkmers, d_state, s); }));
    SkState st;
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_off != ~0ull)
        return fail("read %lld: its offsets do not ascend inside the sequence buffer", static_cast<long long>(st.bad_off) + 1);
    return 0;
}

int sarlacc_dev_sketch_links(const uint64_t* d_sketch, int64_t n, int buckets, int window, int min_shared, uint64_t* d_links,
                             int64_t capacity, int64_t* n_pairs, int64_t* n_links, void* stream) {
    SL_TRY(count_ok(n, "reads"));
    const int lb = buckets_log2(buckets);
    if (lb < 0) return fail("sarlacc_amd: 'buckets' is a power of two in 16 .. 256");
    if (window < 1 || window > 64) return fail("sarlacc_amd: 'window' lies in 1 .. 64");
    if (min_shared < 1 || min_shared > buckets) return fail("sarlacc_amd: 'min_shared' lies in 1 .. buckets");
    if (capacity < 0) return fail("sarlacc_amd: negative capacity");
    const long long m = static_cast<long long>(n) << lb;
    if (m >= SK_LIMIT) return fail("sarlacc_amd: %lld sketch entries (reads x buckets): at most 2^31 - 1 in a call", m);
    if (n_pairs) *n_pairs = 0;
    if (n_links) *n_links = 0;
    ctx().counts["sketch_verify_pairs"] = 0;      // new links: none of them verified yet
    ctx().counts["sketch_verify_second_strand"] = 0;
    if (n < 2) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t count = static_cast<size_t>(m);
    SkState* d_state;
    uint64_t* d_hash;
    int32_t *d_read, *d_sread, *d_count;
    int64_t* d_begin;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("sk.hash", count, &d_hash));
    SL_TRY(scratch("sk.read", count, &d_read));
    SL_TRY(scratch("sk.sread", count, &d_sread));
    SL_TRY(scratch("sk.count", count + 1, &d_count));
    SL_TRY(scratch("sk.begin", count + 1, &d_begin));
    SL_TRY(staged("sketch_entries_sort", s, [&]() -> int {
        SL_TRY(launch_sk_entry_reads(m, lb, d_read, s));
        // stable: entries of equal hash stay in read order; the empty ones sort behind every hash
        return radix_sort_pairs("sk.sort", const_cast<uint64_t*>(d_sketch), d_hash, d_read, d_sread, count, 64, s);
    }));
    long long t = 0;
    const int bits = ceil_log2(static_cast<unsigned long long>(n));
    uint64_t *d_pair = nullptr, *d_spair = nullptr;
    SL_TRY(staged("sketch_pairs", s, [&]() -> int {
        SL_TRY(launch_sk_pairs_count(d_hash, m, window, d_count, s));
        SL_TRY(exclusive_scan("sk.scan", d_count, d_begin, count + 1, s));
        SL_HIP(hipMemcpyAsync(&t, d_begin + m, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        if (t == 0) return 0;
        SL_TRY(scratch("sk.pair", static_cast<size_t>(t), &d_pair));
        SL_TRY(scratch("sk.spair", static_cast<size_t>(t), &d_spair));
        return launch_sk_pairs_fill(d_sread, m, d_begin, bits, d_pair, s);
    }));
    if (t == 0) return 0;
    SL_TRY(staged("sketch_pairs_sort", s, [&] { return radix_sort_keys("sk.sort", d_pair, d_spair, static_cast<size_t>(t), 2 * bits, s); }));
    int32_t* d_flag;
    int64_t* d_before;
    SL_TRY(scratch("sk.flag", static_cast<size_t>(t) + 1, &d_flag));
    SL_TRY(scratch("sk.before", static_cast<size_t>(t) + 1, &d_before));
    SL_TRY(staged("sketch_select", s, [&]() -> int {
        SL_TRY(launch_sk_link_flags(d_spair, t, min_shared, d_flag, d_state, s));
        SL_TRY(exclusive_scan("sk.scan", d_flag, d_before, static_cast<size_t>(t) + 1, s));
        return launch_sk_link_scatter(d_spair, t, bits, d_flag, d_before, d_links, d_links ? capacity : 0, d_state, s);
    }));
    SkState st;
    SL_TRY(state_fetch(d_state, &st, s));
    if (n_pairs) *n_pairs = static_cast<int64_t>(st.n_pairs);
    if (n_links) *n_links = static_cast<int64_t>(st.n_links);
    return 0;
}

int sarlacc_dev_links_verify(const uint8_t* d_seq, const int64_t* d_off, int64_t n, const uint64_t* d_links, int64_t n_links,
                             int bandwidth, int64_t max_diff_ppm, int both_strands, int32_t* d_dist, uint8_t* d_strand,
                             uint64_t* d_kept, int64_t* n_kept, void* stream) {
    SL_TRY(count_ok(n, "reads"));
    SL_TRY(count_ok(n_links, "links"));
    if (bandwidth < 0 || bandwidth > LV_MAX_BANDWIDTH) return fail("sarlacc_amd: 'bandwidth' lies in 0 .. %d", LV_MAX_BANDWIDTH);
    if (max_diff_ppm < 0 || max_diff_ppm >= LV_PPM) return fail("sarlacc_amd: 'max_diff_ppm' lies in 0 .. 999999");
    if (n_kept) *n_kept = 0;
    Context& c = ctx();
    c.counts["sketch_verify_pairs"] = 0;
    c.counts["sketch_verify_second_strand"] = 0;
    if (n_links == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t count = static_cast<size_t>(n_links);
    SkState* d_state;
    int32_t* d_flag;
    int64_t* d_before;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("sk.flag", count + 1, &d_flag));
    SL_TRY(scratch("sk.before", count + 1, &d_before));
    const VerifyArgs a{d_seq, d_off, n, d_links, n_links, bandwidth, max_diff_ppm, both_strands ? 1 : 0};
    SkState st;
    // the stage in two segments: nothing that rests on a refused link or read is launched
    c.stage_reset("sketch_verify");
    SL_TRY(c.stage_begin("sketch_verify", s));
    SL_TRY(launch_links_verify(a, d_dist, d_strand, d_flag, d_state, s));
    SL_TRY(c.stage_end("sketch_verify", s));
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_link != ~0ull) return fail("link %lld: its ends are not 0 <= a < b < n", static_cast<long long>(st.bad_link) + 1);
    if (st.bad_off != ~0ull)
        return fail("read %lld: its offsets do not ascend inside the sequence buffer, or it has 2^31 bases or more", static_cast<long long>(st.bad_off) + 1);
    SL_TRY(c.stage_begin("sketch_verify", s));
    SL_TRY(exclusive_scan("sk.scan", d_flag, d_before, count + 1, s));
    SL_TRY(launch_links_keep(d_links, n_links, d_flag, d_before, d_kept, d_state, s));
    SL_TRY(c.stage_end("sketch_verify", s));
    SL_TRY(state_fetch(d_state, &st, s));
    c.counts["sketch_verify_pairs"] = static_cast<double>(n_links);
    c.counts["sketch_verify_second_strand"] = static_cast<double>(st.n_second);
    if (n_kept) *n_kept = static_cast<int64_t>(st.n_kept);
    return 0;
}

int sarlacc_dev_components(const uint64_t* d_links, int64_t n_links, int64_t n, const int32_t* d_nkmers, int32_t* d_label,
                           int64_t* n_groups, void* stream) {
    SL_TRY(count_ok(n, "vertices"));
    SL_TRY(count_ok(n_links, "links"));
    if (n_groups) *n_groups = 0;
    if (n == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t count = static_cast<size_t>(n);
    SkState* d_state;
    int32_t *d_parent, *d_head, *d_before;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("sk.parent", count, &d_parent));
    SL_TRY(scratch("sk.head", count + 1, &d_head));
    SL_TRY(scratch("sk.rank", count + 1, &d_before));
    SkState st;
    int rounds = 0;
    SL_TRY(staged("components", s, [&]() -> int {
        SL_TRY(launch_cc_init(n, d_parent, s));
        for (bool changed = n_links > 0; changed; ++rounds) {
            SL_HIP(hipMemsetAsync(&d_state->changed, 0, sizeof(unsigned int), s));
            SL_TRY(launch_cc_hook(d_links, n_links, n, d_nkmers, d_parent, d_state, s));
            SL_TRY(launch_cc_jump(n, d_parent, s));
            SL_TRY(state_fetch(d_state, &st, s));
            if (st.bad_link != ~0ull) return 0;
            changed = st.changed != 0;
        }
        SL_TRY(launch_cc_heads(d_parent, d_nkmers, n, d_head, s));
        SL_TRY(exclusive_scan("sk.scan", d_head, d_before, count + 1, s));
        return launch_cc_labels(d_parent, d_nkmers, n, d_before, d_label, d_state, s);
    }));
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_link != ~0ull) return fail("link %lld: an end outside 0 .. n - 1", static_cast<long long>(st.bad_link) + 1);
    ctx().counts["components_rounds"] = rounds;
    if (n_groups) *n_groups = static_cast<int64_t>(st.n_groups);
    return 0;
}
}
