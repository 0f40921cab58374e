// read_groups_host.cpp -- host side of read_groups.hip: argument checks, scratch, the rocPRIM sorts and scans between the
// launches, results, errors and the four C entry points (include/sarlacc_amd.h "pre-groups of a read batch").
//
// Stage timers (sarlacc_stage_ms): names_keys, names_build, names_check, names_probe, records_pick, locus_labels,
// labels_csr.
#include "read_groups.hpp"

#include "devprim.hpp"

#include "../../include/sarlacc_amd.h"

namespace sarlacc {
namespace {

constexpr long long RG_LIMIT = 1LL << 31;

int count_ok(int64_t n, const char* what) {
    if (n < 0) return fail("sarlacc_amd: negative number of %s", what);
    if (n >= RG_LIMIT) return fail("sarlacc_amd: %lld %s: at most 2^31 - 1", static_cast<long long>(n), what);
    return 0;
}

// The call's state block, cleared on the stream.
int state_begin(RgState** d_state, hipStream_t s) {
    SL_TRY(scratch("rg.state", 1, d_state));
    return rg_state_reset(*d_state, s);
}

int state_fetch(const RgState* d_state, RgState* host, hipStream_t s) {
    SL_HIP(hipMemcpyAsync(host, d_state, sizeof(RgState), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

template <typename F>
int staged(const char* name, hipStream_t s, F&& body) {
    Context& c = ctx();
    c.stage_reset(name);
    SL_TRY(c.stage_begin(name, s));
    SL_TRY(body());
    return c.stage_end(name, s);
}

struct MaxI64 {
    __host__ __device__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_names_match(const uint8_t* d_read_names, const int64_t* d_read_off, int64_t n_reads, const uint8_t* d_rec_names,
                            const int64_t* d_rec_off, int64_t n_records, int32_t* d_read_of_record, int64_t* n_unmatched,
                            void* stream) {
    SL_TRY(count_ok(n_reads, "reads"));
    SL_TRY(count_ok(n_records, "records"));
    if (n_unmatched) *n_unmatched = 0;
    if (n_reads == 0 && n_records == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_reads == 0) {      // no key: every record is unmatched
        SL_HIP(hipMemsetAsync(d_read_of_record, 0xff, static_cast<size_t>(n_records) * sizeof(int32_t), s));
        SL_HIP(hipStreamSynchronize(s));
        if (n_unmatched) *n_unmatched = n_records;
        return 0;
    }
    const int hash_bits = option(OPT_NAMES_HASH_BITS);
    if (hash_bits < 0 || hash_bits > 64) return fail("sarlacc_amd: option names_hash_bits is 0 (all bits) or 1 .. 64");
    long long nslots = 64;
    while (nslots < 2 * n_reads) nslots <<= 1;
    RgState* d_state;
    int32_t* d_klen;
    uint64_t *d_hash, *d_table;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("rg.klen", static_cast<size_t>(n_reads), &d_klen));
    SL_TRY(scratch("rg.hash", static_cast<size_t>(n_reads), &d_hash));
    SL_TRY(scratch("rg.table", static_cast<size_t>(nslots), &d_table));
    SL_HIP(hipMemsetAsync(d_table, 0xff, static_cast<size_t>(nslots) * sizeof(uint64_t), s));
    const NameSet reads{d_read_names, d_read_off, n_reads}, recs{d_rec_names, d_rec_off, n_records};
    SL_TRY(staged("names_keys", s, [&] { return launch_name_keys(reads, hash_bits, d_klen, d_hash, d_state, s); }));
    SL_TRY(staged("names_build", s, [&] { return launch_name_build(reads, d_klen, d_hash, d_table, nslots, s); }));
    SL_TRY(staged("names_check", s, [&] { return launch_name_check(reads, d_klen, d_hash, d_table, nslots, d_state, s); }));
    if (n_records)
        SL_TRY(staged("names_probe", s, [&] {
            return launch_name_probe(reads, d_klen, d_table, nslots, recs, hash_bits, d_read_of_record, d_state, s);
        }));
    RgState st;
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_read_off != ~0ull)
        return fail("read name %lld: its offsets do not ascend inside the name buffer", static_cast<long long>(st.bad_read_off) + 1);
    if (st.bad_rec_off != ~0ull)
        return fail("record name %lld: its offsets do not ascend inside the name buffer", static_cast<long long>(st.bad_rec_off) + 1);
    if (st.dup != ~0ull)
        return fail("read names %lld and %lld are the same up to their first space or tab",
                    static_cast<long long>(st.dup & 0xffffffffull) + 1, static_cast<long long>(st.dup >> 32) + 1);
    if (n_unmatched) *n_unmatched = static_cast<int64_t>(st.unmatched);
    return 0;
}

int sarlacc_dev_records_pick(const int32_t* d_read_of_record, const int32_t* d_width, int64_t n_records, int64_t n_reads,
                             int32_t* d_record_of_read, int32_t* d_records_per_read, void* stream) {
    SL_TRY(count_ok(n_reads, "reads"));
    SL_TRY(count_ok(n_records, "records"));
    if (n_reads == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    RgState* d_state;
    unsigned long long* d_best;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("rg.best", static_cast<size_t>(n_reads), &d_best));
    SL_HIP(hipMemsetAsync(d_best, 0, static_cast<size_t>(n_reads) * sizeof(unsigned long long), s));
    SL_HIP(hipMemsetAsync(d_records_per_read, 0, static_cast<size_t>(n_reads) * sizeof(int32_t), s));
    SL_TRY(staged("records_pick", s, [&] {
        return launch_pick(d_read_of_record, d_width, n_records, n_reads, d_best, d_record_of_read, d_records_per_read, d_state, s);
    }));
    RgState st;
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_value != ~0ull)
        return fail("record %lld: a read index outside the batch or a negative width", static_cast<long long>(st.bad_value) + 1);
    return 0;
}

int sarlacc_dev_locus_labels(const int32_t* d_ref, const uint8_t* d_strand, const int32_t* d_start, const int32_t* d_width,
                             int64_t n_records, const int32_t* d_record_of_read, int64_t n_reads, int64_t maxgap, int ignore_strand,
                             int32_t* d_label, int64_t* n_groups, void* stream) {
    SL_TRY(count_ok(n_reads, "reads"));
    SL_TRY(count_ok(n_records, "records"));
    if (maxgap < 0 || maxgap >= RG_LIMIT) return fail("sarlacc_amd: 'maxgap' lies in 0 .. 2^31 - 1");
    if (n_groups) *n_groups = 0;
    if (n_reads == 0) return 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = static_cast<size_t>(n_reads);
    RgState* d_state;
    uint64_t *d_key, *d_skey;
    int32_t *d_idx, *d_sidx, *d_flag, *d_before;
    uint32_t* d_seg;
    int64_t *d_end, *d_runmax;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("rg.lkey", n, &d_key));
    SL_TRY(scratch("rg.lskey", n, &d_skey));
    SL_TRY(scratch("rg.lidx", n, &d_idx));
    SL_TRY(scratch("rg.lsidx", n, &d_sidx));
    SL_TRY(scratch("rg.lseg", n, &d_seg));
    SL_TRY(scratch("rg.lend", n, &d_end));
    SL_TRY(scratch("rg.lrunmax", n, &d_runmax));
    SL_TRY(scratch("rg.flag", n + 1, &d_flag));
    SL_TRY(scratch("rg.before", n + 1, &d_before));
    const LocusArgs a{d_ref, d_strand, d_start, d_width, d_record_of_read, n_records, n_reads, maxgap, ignore_strand ? 1 : 0};
    SL_TRY(staged("locus_labels", s, [&]() -> int {
        SL_TRY(launch_locus_keys(a, d_key, d_idx, d_state, s));
        // stable: reads of equal (reference, strand, start) stay in index order
        SL_TRY(radix_sort_pairs("rg.sort", d_key, d_skey, d_idx, d_sidx, n, 64, s));
        SL_TRY(launch_locus_ends(a, d_skey, d_sidx, d_seg, d_end, s));
        // running maximum of the ends, started anew where the segment changes
        size_t tmp = 0;
        SL_HIP(rocprim::inclusive_scan_by_key(nullptr, tmp, d_seg, d_end, d_runmax, n, MaxI64(), rocprim::equal_to<uint32_t>(), s));
        void* d_tmp;
        SL_TRY(ctx().buffer("rg.scan", tmp ? tmp : 16, &d_tmp));
        SL_HIP(rocprim::inclusive_scan_by_key(d_tmp, tmp, d_seg, d_end, d_runmax, n, MaxI64(), rocprim::equal_to<uint32_t>(), s));
        SL_TRY(launch_locus_flags(a, d_skey, d_seg, d_runmax, d_flag, s));
        SL_TRY(exclusive_scan("rg.scan", d_flag, d_before, n + 1, s));
        return launch_locus_scatter(a, d_skey, d_sidx, d_flag, d_before, d_label, d_state, s);
    }));
    RgState st;
    SL_TRY(state_fetch(d_state, &st, s));
    if (st.bad_value != ~0ull)
        return fail("read %lld: its record lies outside the columns, or has a seqname code outside 0 .. 2^30 - 1 or a negative width",
                    static_cast<long long>(st.bad_value) + 1);
    if (n_groups) *n_groups = st.n_groups;
    return 0;
}

int sarlacc_dev_labels_csr(const int32_t* d_label, int64_t n, int64_t* d_group_off, int32_t* d_members, int64_t* n_groups,
                           int64_t* n_members, void* stream) {
    SL_TRY(count_ok(n, "labels"));
    if (n_groups) *n_groups = 0;
    if (n_members) *n_members = 0;
    SL_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        SL_HIP(hipMemsetAsync(d_group_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    const size_t count = static_cast<size_t>(n);
    RgState* d_state;
    uint32_t *d_key, *d_skey;
    int32_t *d_idx, *d_head, *d_before;
    SL_TRY(state_begin(&d_state, s));
    SL_TRY(scratch("rg.ckey", count, &d_key));
    SL_TRY(scratch("rg.cskey", count, &d_skey));
    SL_TRY(scratch("rg.cidx", count, &d_idx));
    SL_TRY(scratch("rg.flag", count + 1, &d_head));
    SL_TRY(scratch("rg.before", count + 1, &d_before));
    SL_TRY(staged("labels_csr", s, [&]() -> int {
        SL_TRY(launch_csr_keys(d_label, n, d_key, d_idx, s));
        // stable: the members of a group ascend; the unlabelled items sort behind every group
        SL_TRY(radix_sort_pairs("rg.sort", d_key, d_skey, d_idx, d_members, count, 32, s));
        SL_TRY(launch_csr_heads(d_skey, n, d_head, s));
        SL_TRY(exclusive_scan("rg.scan", d_head, d_before, count + 1, s));
        return launch_csr_offsets(d_skey, n, d_head, d_before, d_group_off, d_state, s);
    }));
    RgState st;
    SL_TRY(state_fetch(d_state, &st, s));
    if (n_groups) *n_groups = st.n_groups;
    if (n_members) *n_members = st.n_members;
    return 0;
}
}
