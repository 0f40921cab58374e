// align_host.cpp -- the host side of the quality-weighted DP above run_align (align.hip): the fp64 cost tables and their
// device layout, the batch upload (chunked over PCIe for large calls), the download and string reversal, the reference's
// error order, the read packer and the C entry points.
#include "align_host.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sarlacc {

// Per-column lookup info: which fp64 table a column reads, decided by the
// reference character alone (src/reference_align.cpp:184-212, SURVEY App.B Q2).
int column_info(char r, uint32_t* info) {
    uint32_t code = 7, tmatch, tmis;
    switch (r) {
        case 'A': code = 0; tmatch = 0; tmis = 1; break;
        case 'C': code = 1; tmatch = 0; tmis = 1; break;
        case 'G': code = 2; tmatch = 0; tmis = 1; break;
        case 'T': code = 3; tmatch = 0; tmis = 1; break;
        case 'M': case 'R': case 'W': case 'S': case 'Y': case 'K': tmatch = tmis = 2; break;
        case 'V': case 'H': case 'D': case 'B': tmatch = tmis = 3; break;
        case 'N': tmatch = tmis = 4; break;
        default: return 1;
    }
    *info = code | (tmatch << 8) | (tmis << 16);
    return 0;
}

// (src/reference_align.cpp:21-52) -- built on the host with the host libm so the
// device never evaluates a transcendental on the scoring path.
void build_tables(const double* errors, int n, std::vector<double>& tab) {
    tab.assign(static_cast<size_t>(5) * n, 0.0);
    const double four = 4.0, ratio = four / (four - 1.0);
    auto odds = [&](double g, double e) { return std::log(g * (1 - e) * four + (1 - g) * e * ratio) / M_LN2; };
    for (int q = 0; q < n; ++q) {
        const double e = errors[q];
        tab[0 * n + q] = odds(1.0 / 1.0, e);          // exact, match      (mode 1 match)
        tab[1 * n + q] = odds(1 - 1.0 / 1.0, e);      // exact, mismatch   (mode 1 mismatch)
        tab[2 * n + q] = odds(1 - 1.0 / 2.0, e);      // 2-fold            (mode 2 mismatch)
        tab[3 * n + q] = odds(1.0 / 3.0, e);          // 3-fold            (mode 3 match)
        tab[4 * n + q] = odds(1.0 / 4.0, e);          // N                 (mode 4 match)
    }
}

// Device layout of the cost table: rows of n doubles, addressed as
//     colbase[column] + (read base code * n + quality) * 8          (one add per cell)
// with read base codes 0-3 = ACGT, 4 = anything else.
//   * columns holding A/C/G/T share eight rows "mis mis mis MATCH mis mis mis mis"; the column
//     of reference base r starts 3 - r rows in, so code == r lands on the match row and every
//     other code (including 4) on a mismatch row;
//   * each ambiguity class present in the reference (2-fold, 3-fold, N) gets five identical
//     rows: its score does not depend on the read base (src/reference_align.cpp:184-212).
void build_cost_rows(const std::vector<double>& tab, int n, const uint32_t* colinfo, int R,
                     std::vector<double>& rows, std::vector<uint32_t>& colbase) {
    rows.clear();
    auto append = [&](int t) { rows.insert(rows.end(), tab.begin() + static_cast<size_t>(t) * n, tab.begin() + static_cast<size_t>(t + 1) * n); };
    for (int r = 0; r < 8; ++r) append(r == 3 ? 0 : 1);
    uint32_t class_base[5] = {0, 0, 0, 0, 0};
    colbase.assign(static_cast<size_t>(R) + 1, 0);
    const uint32_t row_bytes = static_cast<uint32_t>(n * sizeof(double));
    for (int col = 1; col <= R; ++col) {
        const uint32_t code = colinfo[col] & 0xff, tmatch = (colinfo[col] >> 8) & 0xff;
        if (code < 4) { colbase[col] = (3 - code) * row_bytes; continue; }
        if (!class_base[tmatch]) {
            class_base[tmatch] = static_cast<uint32_t>(rows.size() * sizeof(double));
            for (int r = 0; r < 5; ++r) append(static_cast<int>(tmatch));
        }
        colbase[col] = class_base[tmatch];
    }
    colbase[0] = colbase[R ? 1 : 0];
}

// Error that the reference would raise first while looping over the reads
// (length mismatch is tested before each alignment, src/adaptor_align.cpp:51-53;
// inside an alignment column 1 is evaluated first: its reference character, then
// the qualities of every row, then the remaining reference characters).
int first_error(int64_t n, const int64_t* seq_off, const int64_t* qual_off, const char* ref, int R,
                int bad_qual_read) {
    int64_t len_bad = -1;
    if (qual_off)
        for (int64_t i = 0; i < n; ++i)
            if (seq_off[i + 1] - seq_off[i] != qual_off[i + 1] - qual_off[i]) { len_bad = i; break; }
    int first_bad_col = -1;
    uint32_t tmp;
    for (int col = 0; col < R; ++col)
        if (column_info(ref[col], &tmp)) { first_bad_col = col; break; }
    int64_t first_nonempty = -1;
    if (first_bad_col >= 0)
        for (int64_t i = 0; i < n; ++i)
            if (seq_off[i + 1] - seq_off[i] > 0) { first_nonempty = i; break; }

    const int64_t INF = std::numeric_limits<int64_t>::max();
    const int64_t e_len = len_bad >= 0 ? len_bad : INF;
    const int64_t e_qual = (R > 0 && bad_qual_read != std::numeric_limits<int>::max()) ? bad_qual_read : INF;
    const int64_t e_ref = first_nonempty >= 0 ? first_nonempty : INF;
    const int64_t first = std::min(e_len, std::min(e_qual, e_ref));
    if (first == INF) return 0;
    if (first == e_len) return fail("sequence and quality strings should have the same length");
    if (first == e_ref && first_bad_col == 0) return fail("unrecognized base in reference sequence");
    if (first == e_qual) return fail("quality cannot be lower than smallest encoded value");
    return fail("unrecognized base in reference sequence");
}

// Uploads a batch given host string sets.  Reads whose quality string has a
// different length make the whole call fail later (first_error), so qualities
// are copied with the sequence offsets only when every length agrees.
int upload_batch(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off,
                 int64_t n, HostBatch* hb, hipStream_t s, bool defer_data) {
    int64_t mx = 0;
    bool same = true;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = seq_off[i + 1] - seq_off[i];
        mx = std::max(mx, L);
        if (L != qual_off[i + 1] - qual_off[i]) { same = false; if (hb->len_bad < 0) hb->len_bad = i; }
    }
    if (mx > std::numeric_limits<int32_t>::max() / 2) return fail("sarlacc_amd: read longer than 2^30 bases");
    hb->max_len = static_cast<int32_t>(mx);
    if (!same) return 0;
    const int64_t base = n ? seq_off[0] : 0;
    const int64_t total = n ? seq_off[n] - base : 0;
    std::vector<int64_t> rel(static_cast<size_t>(n) + 1);
    for (int64_t i = 0; i <= n; ++i) rel[i] = (n ? seq_off[i] : 0) - base;
    if (defer_data) {   // the caller copies the bases and qualities chunk by chunk
        SL_TRY(scratch("batch.seq", static_cast<size_t>(total), &hb->d_seq));
        SL_TRY(scratch("batch.qual", static_cast<size_t>(total), &hb->d_qual));
    } else {
        SL_TRY(upload("batch.seq", reinterpret_cast<const uint8_t*>(seq) + base, static_cast<size_t>(total), &hb->d_seq, s));
        SL_TRY(upload("batch.qual", reinterpret_cast<const uint8_t*>(qual) + (n ? qual_off[0] : 0), static_cast<size_t>(total), &hb->d_qual, s));
    }
    SL_TRY(upload("batch.off", rel.data(), rel.size(), &hb->d_off, s));
    if (defer_data) SL_HIP(hipStreamSynchronize(s));   // `rel` goes out of scope
    return 0;
}

static int check_sections(const int32_t* ss, const int32_t* se, int nsec, int R) {
    for (int x = 0; x < nsec; ++x)
        if (ss[x] < 0 || ss[x] > R || se[x] < 0 || se[x] > R)
            return fail("sarlacc_amd: section bounds outside the adaptor (the reference reads out of range here)");
    return 0;
}

// Where a host-pointer call wants its results (null: not asked for)
struct HostOut {
    double* scores = nullptr;
    int32_t *starts = nullptr, *ends = nullptr, *sec_so = nullptr, *sec_wo = nullptr, *edits = nullptr;   // kernel mode 1; edits: mode 2 ...
    char *aln_ref = nullptr, *aln_qry = nullptr;   // ... and its strings, unless edits only
    int64_t *aln_off = nullptr, aln_cap = 0;
};

// `job` comes with everything but its batch, outputs and stream: those are the device copies made here.
static int host_align(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t n, AlignJob job,
                      const HostOut& ho) {
    const int R = job.R, kernel_mode = job.kernel_mode, nsec = job.nsec;
    AlignOut& out = job.out;
    SL_TRY(check_encoding(job.sc.enc_errors, job.sc.enc_names, job.sc.enc_n));
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    if (kernel_mode == 1) SL_TRY(check_sections(job.sec_starts, job.sec_ends, nsec, R));
    SL_TRY(ensure_device());
    hipStream_t s = nullptr;
    if (n == 0) { if (ho.aln_off) ho.aln_off[0] = 0; return 0; }

    // Large score / map calls go to the device in chunks: the bases and qualities of chunk k+1
    // cross PCIe on a stream of their own while chunk k is aligned.
    const int64_t total_bytes = seq_off[n] - seq_off[0];
    int64_t nchunks = 1;
    if (kernel_mode != 2 && R > 0) {
        if (total_bytes >= (static_cast<int64_t>(512) << 20)) nchunks = std::min<int64_t>(8, total_bytes / (static_cast<int64_t>(256) << 20));
        if (option(OPT_ALIGN_CHUNKS) > 0) nchunks = option(OPT_ALIGN_CHUNKS);   // testing
        nchunks = std::max<int64_t>(1, std::min<int64_t>(nchunks, n));
    }
    HostBatch hb;
    SL_TRY(upload_batch(seq, seq_off, qual, qual_off, n, &hb, s, nchunks > 1));
    if (hb.len_bad >= 0) {
        // reads before the offending one could still raise an earlier error, but
        // only a bad reference character is detectable without the qualities
        return first_error(n, seq_off, qual_off, job.ref, R, std::numeric_limits<int>::max());
    }
    const size_t nn = static_cast<size_t>(n);
    SL_TRY(scratch("out.scores", nn, &out.d_scores));
    if (kernel_mode == 1) {
        SL_TRY(scratch("out.starts", nn, &out.d_starts));
        SL_TRY(scratch("out.ends", nn, &out.d_ends));
        SL_TRY(scratch("out.sso", nn * std::max(nsec, 1), &out.d_sec_so));
        SL_TRY(scratch("out.swo", nn * std::max(nsec, 1), &out.d_sec_wo));
    }
    const size_t aln_bytes = static_cast<size_t>(total_bytes + n * R);
    if (kernel_mode == 2) {
        SL_TRY(scratch("out.aref", aln_bytes, &out.d_aln_ref));
        SL_TRY(scratch("out.aqry", aln_bytes, &out.d_aln_qry));
        SL_TRY(scratch("out.alen", nn, &out.d_aln_len));
        SL_TRY(scratch("out.edits", nn, &out.d_edits));
    }
    job.batch = {hb.d_seq, hb.d_qual, hb.d_off, n, hb.max_len}; job.stream = s;
    int bad = 0;
    if (nchunks == 1) {
        SL_TRY(run_align(job, &bad));
    } else {
        hipStream_t copy_stream = nullptr;
        SL_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        std::vector<hipEvent_t> ready(static_cast<size_t>(nchunks), nullptr);
        const int64_t sbase = seq_off[0], qbase = qual_off[0];
        auto bound = [&](int64_t k) { return n * k / nchunks; };
        auto send = [&](int64_t k) -> int {   // bases and qualities of the reads of chunk k
            const int64_t lo = seq_off[bound(k)] - sbase, hi = seq_off[bound(k + 1)] - sbase;
            if (hi > lo) {
                SL_HIP(hipMemcpyAsync(hb.d_seq + lo, seq + sbase + lo, static_cast<size_t>(hi - lo), hipMemcpyHostToDevice, copy_stream));
                SL_HIP(hipMemcpyAsync(hb.d_qual + lo, qual + qbase + lo, static_cast<size_t>(hi - lo), hipMemcpyHostToDevice, copy_stream));
            }
            SL_HIP(hipEventCreateWithFlags(&ready[k], hipEventDisableTiming));
            SL_HIP(hipEventRecord(ready[k], copy_stream));
            return 0;
        };
        int rc = send(0);
        for (int64_t k = 0; k < nchunks && !rc; ++k) {
            const int64_t lo = bound(k), hi = bound(k + 1);
            rc = hipStreamWaitEvent(s, ready[k], 0) == hipSuccess ? 0 : fail("HIP error waiting for a chunk upload");
            if (rc) break;
            AlignJob cj = job;
            cj.batch.d_off = hb.d_off + lo; cj.batch.n = hi - lo;
            cj.out.d_scores = out.d_scores + lo;
            if (out.d_starts) { cj.out.d_starts = out.d_starts + lo; cj.out.d_ends = out.d_ends + lo; }
            if (out.d_sec_so) { cj.out.d_sec_so = out.d_sec_so + lo; cj.out.d_sec_wo = out.d_sec_wo + lo; }
            ChunkOpts co;
            co.sec_stride = n; co.read_base = static_cast<int>(lo); co.init_bad = (k == 0); co.finish = (k + 1 == nchunks);
            rc = run_align(cj, &bad, co);
            if (!rc && k + 1 < nchunks) rc = send(k + 1);   // travels while chunk k is being aligned
        }
        (void)hipStreamSynchronize(copy_stream);
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ready) if (e) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(copy_stream);
        if (rc) return rc;
    }
    SL_TRY(first_error(n, seq_off, nullptr, job.ref, R, bad));

    SL_HIP(hipMemcpy(ho.scores, out.d_scores, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (kernel_mode == 1) {
        SL_HIP(hipMemcpy(ho.starts, out.d_starts, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
        SL_HIP(hipMemcpy(ho.ends, out.d_ends, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (nsec) {
            SL_HIP(hipMemcpy(ho.sec_so, out.d_sec_so, nn * nsec * sizeof(int32_t), hipMemcpyDeviceToHost));
            SL_HIP(hipMemcpy(ho.sec_wo, out.d_sec_wo, nn * nsec * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
    }
    if (kernel_mode == 2) {
        SL_HIP(hipMemcpy(ho.edits, out.d_edits, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ho.aln_ref) {
            std::vector<uint8_t> hr(aln_bytes), hq(aln_bytes);
            std::vector<int32_t> hl(nn);
            SL_HIP(hipMemcpy(hr.data(), out.d_aln_ref, aln_bytes, hipMemcpyDeviceToHost));
            SL_HIP(hipMemcpy(hq.data(), out.d_aln_qry, aln_bytes, hipMemcpyDeviceToHost));
            SL_HIP(hipMemcpy(hl.data(), out.d_aln_len, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
            int64_t used = 0;
            ho.aln_off[0] = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t base = (seq_off[i] - seq_off[0]) + i * static_cast<int64_t>(R);
                const int32_t m = hl[i];
                if (used + m > ho.aln_cap) return fail("sarlacc_amd: alignment string buffer too small");
                for (int32_t x = 0; x < m; ++x) {  // the device wrote them end-first
                    ho.aln_ref[used + x] = static_cast<char>(hr[base + m - 1 - x]);
                    ho.aln_qry[used + x] = static_cast<char>(hq[base + m - 1 - x]);
                }
                used += m;
                ho.aln_off[i + 1] = used;
            }
        }
    }
    return 0;
}

}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_adaptor_align(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off,
                          int64_t n, const double* enc_errors, const char* enc_names, int enc_n, double gapopen,
                          double gapext, const char* adaptor, int adaptor_len, const int32_t* sec_starts,
                          const int32_t* sec_ends, int nsec, double* scores, int32_t* starts, int32_t* ends,
                          int32_t* sec_start_out, int32_t* sec_width_out) {
    const AlignJob job{{}, {enc_errors, enc_names, enc_n, gapopen, gapext}, adaptor, adaptor_len, true, 1, sec_starts, sec_ends, nsec};
    return host_align(seq, seq_off, qual, qual_off, n, job, {scores, starts, ends, sec_start_out, sec_width_out});
}

int sarlacc_adaptor_align_score_only(const char* seq, const int64_t* seq_off, const char* qual,
                                     const int64_t* qual_off, int64_t n, const double* enc_errors,
                                     const char* enc_names, int enc_n, double gapopen, double gapext,
                                     const char* adaptor, int adaptor_len, double* scores) {
    const AlignJob job{{}, {enc_errors, enc_names, enc_n, gapopen, gapext}, adaptor, adaptor_len, true, 0};
    return host_align(seq, seq_off, qual, qual_off, n, job, {scores});
}

int sarlacc_barcode_align(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off,
                          int64_t n, const double* enc_errors, const char* enc_names, int enc_n, double gapopen,
                          double gapext, const char* reference, int reference_len, double* scores) {
    const AlignJob job{{}, {enc_errors, enc_names, enc_n, gapopen, gapext}, reference, reference_len, false, 0};
    return host_align(seq, seq_off, qual, qual_off, n, job, {scores});
}

int sarlacc_general_align(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off,
                          int64_t n, const double* enc_errors, const char* enc_names, int enc_n, double gapopen,
                          double gapext, const char* reference, int reference_len, int edit_only, double* scores,
                          int32_t* edits, char* aln_ref, char* aln_query, int64_t* aln_off, int64_t aln_cap) {
    const AlignJob job{{}, {enc_errors, enc_names, enc_n, gapopen, gapext}, reference, reference_len, false, 2};
    HostOut ho{scores};
    ho.edits = edits; ho.aln_off = aln_off; ho.aln_cap = aln_cap;
    if (!edit_only) { ho.aln_ref = aln_ref; ho.aln_qry = aln_query; }
    return host_align(seq, seq_off, qual, qual_off, n, job, ho);
}

// `job` comes with the sections as the caller gave them: they count only where positions are asked for.
static int dev_align_impl(AlignJob job, int mode) {
    SL_TRY(check_encoding(job.sc.enc_errors, job.sc.enc_names, job.sc.enc_n));
    SL_TRY(ensure_device());
    const bool trace = job.out.d_starts != nullptr;
    if (trace && mode != 0) return fail("sarlacc_amd: positions are only defined for the local (adaptor) mode");
    if (trace) SL_TRY(check_sections(job.sec_starts, job.sec_ends, job.nsec, job.R));
    job.kernel_mode = trace ? 1 : 0; job.nsec = trace ? job.nsec : 0;
    int bad = 0;
    SL_TRY(run_align(job, &bad));
    if (job.R > 0 && bad != std::numeric_limits<int>::max())
        return fail("quality cannot be lower than smallest encoded value");
    uint32_t tmp;
    for (int col = 0; col < job.R; ++col)
        if (column_info(job.ref[col], &tmp) && job.batch.max_len > 0) return fail("unrecognized base in reference sequence");
    return 0;
}

// 8 bases per thread: 2 bytes of 2-bit codes + 1 byte of exception bits
__global__ void k_pack_reads(const uint8_t* seq, long long total, uint8_t* packed, uint8_t* nmask) {
    const long long o = (blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x) * 8;
    if (o >= total) return;
    uint32_t bits = 0, exc = 0;
    for (int k = 0; k < 8; ++k) {
        const uint8_t c = (o + k < total) ? seq[o + k] : static_cast<uint8_t>('A');
        uint32_t v;
        switch (c) {
            case 'A': v = 0; break;
            case 'C': v = 1; break;
            case 'G': v = 2; break;
            case 'T': v = 3; break;
            default: v = 0; exc |= 1u << k; break;
        }
        bits |= v << (2 * k);
    }
    packed[o / 4] = static_cast<uint8_t>(bits);
    packed[o / 4 + 1] = static_cast<uint8_t>(bits >> 8);  // the buffer has one spare byte
    nmask[o / 8] = static_cast<uint8_t>(exc);
}

int sarlacc_dev_pack_reads(const uint8_t* d_seq, int64_t total, uint8_t* d_packed, uint8_t* d_nmask, void* stream) {
    if (total < 0) return fail("sarlacc_amd: negative size");
    if (total == 0) return 0;
    SL_TRY(ensure_device());
    const long long threads = (total + 7) / 8;
    hipLaunchKernelGGL(k_pack_reads, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_seq, static_cast<long long>(total), d_packed, d_nmask);
    SL_HIP(hipGetLastError());
    return 0;
}

int sarlacc_dev_align(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                      int32_t max_len, const double* enc_errors, const char* enc_names, int enc_n, double gapopen,
                      double gapext, const char* reference, int reference_len, int mode, const int32_t* sec_starts,
                      const int32_t* sec_ends, int nsec, double* d_scores, int32_t* d_starts, int32_t* d_ends,
                      int32_t* d_sec_start_out, int32_t* d_sec_width_out, void* stream) {
    return dev_align_impl({{d_seq, d_qual, d_off, n, max_len}, {enc_errors, enc_names, enc_n, gapopen, gapext}, reference, reference_len, mode == 0, 0, sec_starts,
                           sec_ends, nsec, {d_scores, d_starts, d_ends, d_sec_start_out, d_sec_width_out}, static_cast<hipStream_t>(stream)}, mode);
}

int sarlacc_dev_align_packed(const uint8_t* d_packed, const uint8_t* d_nmask, const uint8_t* d_qual,
                             const int64_t* d_off, int64_t n, int32_t max_len, const double* enc_errors,
                             const char* enc_names, int enc_n, double gapopen, double gapext, const char* reference,
                             int reference_len, int mode, const int32_t* sec_starts, const int32_t* sec_ends, int nsec,
                             double* d_scores, int32_t* d_starts, int32_t* d_ends, int32_t* d_sec_start_out,
                             int32_t* d_sec_width_out, void* stream) {
    if (!d_nmask) return fail("sarlacc_amd: packed alignment needs the exception mask of sarlacc_dev_pack_reads");
    return dev_align_impl({{d_packed, d_qual, d_off, n, max_len, d_nmask}, {enc_errors, enc_names, enc_n, gapopen, gapext}, reference, reference_len, mode == 0, 0,
                           sec_starts, sec_ends, nsec, {d_scores, d_starts, d_ends, d_sec_start_out, d_sec_width_out}, static_cast<hipStream_t>(stream)}, mode);
}
}
