// consensus_host.cpp -- host side of the consensus vote (kernels and their launches: consensus.hip; shared: consensus.hpp).
//
// consensus_core runs one call as a sequence: plan (which kernels, with what LDS and geometry) -> tables (host libm) ->
// rows and scratch -> vote -> read back -> first error in the reference's order -> the vote again while the boundary
// list was too short -> compact -> host-libm fix-up of the boundary columns.  Its two callers build the job:
// run_consensus from alignments in host memory (reference src/create_consensus.cpp:150-170, :287-308), msa_consensus_impl
// from the rows the MSA stage left in HBM.  cons_plan, cons_codes_allowed, cons_tables, check_structure, first_error and
// apply_fixes are plain host code over host values: no HIP call.
#include "consensus.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace sarlacc {

// ---------------------------------------------------------------------------
// Route plan

constexpr size_t CONS_ROW_RECORD = 2 * sizeof(long long) + 3 * sizeof(int);   // LDS per row of an alignment: row and quality offsets, position, flag, quality length
constexpr size_t CONS_LDS_PLAIN = 48 * 1024;    // dynamic LDS a kernel takes as it stands; k_consensus_q4 (4 workgroups per CU) never gets more
constexpr size_t CONS_LDS_STRIP = 150 * 1024;   // the strip table of k_consensus_qf / k_consensus_code: one workgroup per CU
constexpr size_t CONS_LDS_MAX = 160 * 1024;     // the LDS of a CU: what the row records of the one-column kernel may take

static size_t rows_lds(int alignments, int max_rows) { return alignments * CONS_ROW_RECORD * static_cast<size_t>(max_rows) + 16; }
static bool lds_plain(size_t bytes) { return bytes <= CONS_LDS_PLAIN; }
static bool strip_fits(int enc_n, int row_bytes) { return static_cast<size_t>(enc_n + 1) * row_bytes <= CONS_LDS_STRIP; }
// the byte-parallel index arithmetic of k_consensus_qf and the 16-bit codes take the first name + enc_n as a byte
static bool names_end_in_byte(int qoffset, int enc_n) { return qoffset + enc_n <= 255; }

// What decides a call's kernels.  (The fused call asks cons_codes_allowed before the MSA stage runs: the fields from
// max_rows on are not known then and not read.)
struct ConsShape {
    bool quality = false;
    bool want_lerr = false;     // the caller wants the per-column log errors
    bool codes = false;         // the rows came as vote codes
    int enc_n = 0, qoffset = 0; // the encoding: entries, first name (a signed char)
    int opt_chars = 0, opt_generic = 0;   // OPT_CONSENSUS_CHARS, OPT_CONSENSUS_GENERIC
    int max_rows = 1;
    long long aln_bytes = 0, qual_bytes = 0, ng_eval = 0;
    int num_cu = 0;
};

// May the MSA stage write the rows as vote codes (k_consensus_code)?  The table has to fit LDS.  (The caller adds what
// takes the reads: every read as long as its quality string, which is also what the reference demands.)
static bool cons_codes_allowed(const ConsShape& in) {
    return in.quality && strip_fits(in.enc_n, QC_ROWB) && names_end_in_byte(in.qoffset, in.enc_n) && !in.opt_chars;
}

static ConsPlan cons_plan(const ConsShape& in) {
    ConsPlan p;
    const size_t n = static_cast<size_t>(in.enc_n);
    const long long cus = in.num_cu;
    // one column per lane, one alignment per wavefront: right / wrong and the row records
    const size_t lds1 = (in.quality ? 2 * sizeof(double) * n : 0) + rows_lds(1, in.max_rows);
    // quality vote without the per-column log errors: 4 columns per lane, 4 alignments per workgroup
    const size_t lds4 = sizeof(double) * 4 * (5 * n + 1) + rows_lds(4, in.max_rows);
    // one 1024-thread workgroup per CU, a wavefront per alignment
    const unsigned grid_strip = static_cast<unsigned>(std::min<long long>((in.ng_eval + QF_THREADS / 64 - 1) / (QF_THREADS / 64), cus));
    p.refused = in.ng_eval > 0 && lds1 > CONS_LDS_MAX;
    if (in.codes) {
        p.route = CONS_CODE;
        p.vote = {(n + 1) * QC_ROWB, grid_strip, QF_THREADS, true};
    } else if (in.quality && !in.want_lerr && lds_plain(lds4)) {
        // (k_consensus_qf's byte-parallel index arithmetic -- QOFF4, QZERO4, KHI -- takes the first name and first name + enc_n as
        // bytes 0..255: a table whose names start at or above byte 128, a negative signed char, goes to k_consensus_q4)
        const bool qf = in.aln_bytes > 0 && in.qual_bytes > 0 && in.enc_n <= 127 && in.qoffset >= 0 && names_end_in_byte(in.qoffset, in.enc_n) &&
                        strip_fits(in.enc_n, QF_ROWB) && !in.opt_generic;
        p.route = qf ? CONS_QF_Q4 : CONS_Q4;
        if (qf) p.qf = {(n + 1) * QF_ROWB, grid_strip, QF_THREADS, true};
        p.vote = {lds4, static_cast<unsigned>(std::min<long long>((in.ng_eval + 3) / 4, cus * 64)), 256, false};
    } else {
        p.route = in.quality ? CONS_GENERIC : CONS_BASIC;
        // (alignments of thousands of rows: more than the default 64 KB of dynamic LDS)
        p.vote = {lds1, static_cast<unsigned>(std::min<long long>(in.ng_eval, cus * 32)), 64, !lds_plain(lds1)};
    }
    return p;
}

// ---------------------------------------------------------------------------
// Tables

// What the route's kernels read of the encoding: k_consensus<true> right / wrong, k_consensus_q4 vec, k_consensus_qf strip,
// k_consensus_code strip8; the others stay empty.
struct ConsTables { std::vector<double> right, wrong, vec, strip, strip8; };

// LDS table of k_consensus_qf (width QF_STRIP) and k_consensus_code (CODE_STRIP): per quality the strip (w w w r w ...)
// of log(e/3) and log1p(-e), every double replicated for QF_SLOTS lanes; a zero row last
static std::vector<double> strip_table(int width, const std::vector<double>& right, const std::vector<double>& wrong) {
    const size_t n = right.size();
    std::vector<double> strip((n + 1) * width * QF_SLOTS, 0.0);
    for (size_t k = 0; k < n; ++k)
        for (int i = 0; i < width; ++i)
            for (int sl = 0; sl < QF_SLOTS; ++sl) strip[(k * width + i) * QF_SLOTS + sl] = (i == 3) ? right[k] : wrong[k];
    return strip;
}

static ConsTables cons_tables(const double* enc_errors, int enc_n, ConsRoute route) {
    ConsTables t;
    if (route == CONS_BASIC) return t;
    std::vector<double> right(enc_n), wrong(enc_n);
    for (int k = 0; k < enc_n; ++k) {  // (src/create_consensus.cpp:14,:218-226)
        double e = enc_errors[k];
        if (e > 0.99999999) e = 0.99999999;
        else if (e < 0.00000001) e = 0.00000001;
        right[k] = std::log1p(-e);
        wrong[k] = std::log(e / 3);
    }
    if (route == CONS_Q4 || route == CONS_QF_Q4) {
        // what a cell adds to (A, C, G, T) by read character (A, C, G, T, other) and quality; the last entry (gap, N, no
        // quality left) adds nothing
        t.vec.assign(static_cast<size_t>(5 * enc_n + 1) * 4, 0.0);
        for (int code = 0; code < 5; ++code)
            for (int k = 0; k < enc_n; ++k)
                for (int bidx = 0; bidx < 4; ++bidx)
                    t.vec[(static_cast<size_t>(code) * enc_n + k) * 4 + bidx] = (bidx == code) ? right[k] : wrong[k];
    }
    if (route == CONS_QF_Q4) t.strip = strip_table(QF_STRIP, right, wrong);
    if (route == CONS_CODE) t.strip8 = strip_table(CODE_STRIP, right, wrong);
    if (route == CONS_GENERIC) { t.right = std::move(right); t.wrong = std::move(wrong); }
    return t;
}

static int upload_tables(const ConsTables& t, ConsArgs& a, hipStream_t s) {
    const struct { const char* name; const std::vector<double>& host; const double*& dev; } tables[] = {
        {"cons.right", t.right, a.right}, {"cons.wrong", t.wrong, a.wrong}, {"cons.vec", t.vec, a.vec},
        {"cons.strip", t.strip, a.strip}, {"cons.strip8", t.strip8, a.strip8}};
    for (const auto& tb : tables) {
        if (tb.host.empty()) continue;
        double* d;
        SL_TRY(upload(tb.name, tb.host.data(), tb.host.size(), &d, s));
        tb.dev = d;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// The job

// The row table of the alignments: row offsets from the first row (rel, one entry past the last row, which is the rows'
// byte count), first row of every group (grows, ngroups + 1 entries), output offset of every group, rows of the deepest group.
struct ConsRows {
    std::vector<int64_t> rel, grows, out_off;
    int max_rows = 1;
};

// ... of alignments given by row offsets and a group table; max_rows over the first `walked` groups (those the structural
// check walked)
static ConsRows rows_from_offsets(const int64_t* aln_off, const int64_t* grp_rows, int64_t ngroups, int64_t walked) {
    ConsRows t;
    const int64_t nrows = grp_rows[ngroups], base = aln_off[0];
    t.rel.resize(static_cast<size_t>(nrows) + 1);
    for (int64_t r = 0; r <= nrows; ++r) t.rel[r] = aln_off[r] - base;
    t.grows.assign(grp_rows, grp_rows + ngroups + 1);
    t.out_off.resize(static_cast<size_t>(std::max<int64_t>(ngroups, 1)));
    for (int64_t g = 0; g < ngroups; ++g) t.out_off[g] = t.rel[grp_rows[g]];
    for (int64_t g = 0; g < walked; ++g) t.max_rows = static_cast<int>(std::max<int64_t>(t.max_rows, grp_rows[g + 1] - grp_rows[g]));
    return t;
}

// ... of the alignments the MSA stage left in HBM: group g has grp_off[g + 1] - grp_off[g] rows of res.width[g] cells from res.out_off[g]
static ConsRows rows_from_widths(const int64_t* grp_off, const MsaResult& res, int64_t ngroups) {
    ConsRows t;
    const int64_t nrows = grp_off[ngroups] - grp_off[0];
    t.rel.resize(static_cast<size_t>(nrows) + 1);
    t.grows.resize(static_cast<size_t>(ngroups) + 1);
    t.out_off.resize(static_cast<size_t>(ngroups));
    int64_t row = 0;
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t m = grp_off[g + 1] - grp_off[g];
        t.grows[g] = row;
        t.out_off[g] = res.out_off[g];
        t.max_rows = static_cast<int>(std::max<int64_t>(t.max_rows, m));
        for (int64_t r = 0; r < m; ++r) t.rel[row++] = res.out_off[g] + r * res.width[g];
    }
    t.grows[ngroups] = row;
    t.rel[nrows] = res.out_off[ngroups];
    return t;
}

// first structural error of the input, found on the host before anything runs; reported after the errors of the groups before it
enum ConsStructErr { CONS_STRUCT_OK, CONS_ROW_WIDTHS_DIFFER, CONS_ENTRY_COUNTS_DIFFER };

struct ConsJob {
    bool quality = false;
    ConsArgs a{};               // in: aln and, where they apply, qual, qual_off, qual_bytes, row_read, codes, code_bad (device pointers)
    int64_t ngroups = 0;        // of the call
    int64_t ng_eval = 0;        // groups before the first structural error: what the device evaluates
    int64_t rows_eval = 0;      // their rows
    int64_t total = 0;          // cells of all rows
    ConsRows rows;
    double min_cov = 0, pseudo = 0;
    const double* enc_errors = nullptr;
    const char* enc_names = nullptr;
    int enc_n = 0;
    char* cons = nullptr;       // the caller's buffers: kept columns, group after group
    char* phred = nullptr;
    int64_t* cons_off = nullptr;
    double* lerr = nullptr;     // optional
    int64_t cons_cap = -1;      // capacity of cons / phred (-1: as large as the input)
    const char* aln_host = nullptr;   // optional host copy of the rows, used only to quote an unknown character
    ConsStructErr struct_err = CONS_STRUCT_OK;
    hipStream_t s = nullptr;
};

static int upload_rows(const ConsRows& t, ConsArgs& a, hipStream_t s) {
    int64_t* d_aoff; int64_t* d_grows; int64_t* d_ooff;
    SL_TRY(upload("cons.aoff", t.rel.data(), t.rel.size(), &d_aoff, s));
    SL_TRY(upload("cons.grows", t.grows.data(), t.grows.size(), &d_grows, s));
    SL_TRY(upload("cons.ooff", t.out_off.data(), t.out_off.size(), &d_ooff, s));
    a.aln_off = d_aoff; a.grp_rows = d_grows; a.out_off = d_ooff; a.max_rows = t.max_rows; a.aln_bytes = t.rel.back();
    return 0;
}

// ---------------------------------------------------------------------------
// Scratch

// the boundary list: cap empty entries (no group recorded)
static int fix_list(ConsArgs& a, int cap, hipStream_t s) {
    SL_TRY(scratch("cons.fixpos", static_cast<size_t>(cap), &a.fix_pos));
    SL_TRY(scratch("cons.fixval", 4 * static_cast<size_t>(cap), &a.fix_val));
    SL_TRY(scratch("cons.fixgrp", static_cast<size_t>(cap), &a.fix_grp));
    SL_HIP(hipMemsetAsync(a.fix_count, 0, sizeof(int), s));
    SL_HIP(hipMemsetAsync(a.fix_grp, 0xff, sizeof(int) * static_cast<size_t>(cap), s));
    a.fix_cap = cap;
    return 0;
}

// the vote's outputs (uncompacted: a column's slot is its cell in the group's first row), flags and the first boundary list
static int vote_scratch(const ConsJob& j, ConsArgs& a) {
    const size_t total = static_cast<size_t>(j.total), nstatus = static_cast<size_t>(std::max<int64_t>(j.rows_eval, 1));
    SL_TRY(scratch("cons.out", total, &a.cons));
    SL_TRY(scratch("cons.phred", total, &a.phred));
    a.lerr = nullptr;
    if (j.lerr) SL_TRY(scratch("cons.lerr", total, &a.lerr));
    SL_TRY(scratch("cons.len", static_cast<size_t>(j.ngroups), &a.cons_len));
    SL_TRY(scratch("cons.status", nstatus, &a.row_status));
    SL_TRY(scratch("cons.badchar", 1, &a.first_bad_char));
    SL_TRY(scratch("cons.fixn", 1, &a.fix_count));
    SL_TRY(scratch("cons.gflag", static_cast<size_t>(std::max<int64_t>(j.ngroups, 1)), &a.gflag));
    SL_HIP(hipMemsetAsync(a.row_status, 0, nstatus, j.s));
    SL_HIP(hipMemsetAsync(a.first_bad_char, 0xff, sizeof(unsigned long long), j.s));
    a.only_flagged = 0;
    return fix_list(a, 4096, j.s);
}

// ---------------------------------------------------------------------------
// Results and errors

struct ConsOutcome {
    std::vector<int32_t> len;       // kept columns per group
    std::vector<int8_t> status;     // per row (ConsArgs::row_status)
    unsigned long long badchar = ~0ull;   // basic vote: byte index of the first unknown character
    char bad = '?';                 // ... and the character
    int code_bad_row = INT_MAX;     // vote codes: smallest row with a quality below the encoding
    int fixn = 0;                   // boundary columns the kernels counted
};

static int read_back(const ConsJob& j, const ConsArgs& a, ConsOutcome& o) {
    const size_t nstatus = static_cast<size_t>(std::max<int64_t>(j.rows_eval, 1));
    o.len.assign(static_cast<size_t>(j.ngroups), 0);
    o.status.assign(nstatus, 0);
    if (j.ng_eval > 0) {
        SL_HIP(hipMemcpy(o.len.data(), a.cons_len, sizeof(int32_t) * static_cast<size_t>(j.ng_eval), hipMemcpyDeviceToHost));
        SL_HIP(hipMemcpy(o.status.data(), a.row_status, nstatus, hipMemcpyDeviceToHost));
        SL_HIP(hipMemcpy(&o.badchar, a.first_bad_char, sizeof o.badchar, hipMemcpyDeviceToHost));
        SL_HIP(hipMemcpy(&o.fixn, a.fix_count, sizeof o.fixn, hipMemcpyDeviceToHost));
    }
    if (!j.quality && o.badchar != ~0ull) {
        if (j.aln_host) o.bad = j.aln_host[static_cast<int64_t>(o.badchar)];
        else SL_HIP(hipMemcpy(&o.bad, a.aln + o.badchar, 1, hipMemcpyDeviceToHost));
    }
    if (a.codes && a.code_bad) SL_HIP(hipMemcpy(&o.code_bad_row, a.code_bad, sizeof o.code_bad_row, hipMemcpyDeviceToHost));
    return 0;
}

// earliest error in the reference's processing order (0: none)
static int first_error(const ConsJob& j, const ConsOutcome& o) {
    if (!j.quality && o.badchar != ~0ull) {
        char msg[96];
        snprintf(msg, sizeof msg, "unknown character '%c' in alignment string", o.bad);
        return fail("%s", msg);
    }
    if (o.code_bad_row != INT_MAX) return fail("quality cannot be lower than smallest encoded value");
    if (j.quality)
        for (int64_t r = 0; r < j.rows_eval; ++r) {
            if (o.status[r] == 1) return fail("quality cannot be lower than smallest encoded value");
            if (o.status[r] == 2) return fail("quality vector is shorter than the alignment sequence");
            if (o.status[r] == 3) return fail("quality vector is longer than the alignment sequence");
        }
    if (j.struct_err == CONS_ROW_WIDTHS_DIFFER) return fail("alignment strings should have the same length");
    if (j.struct_err == CONS_ENTRY_COUNTS_DIFFER) return fail("alignments and qualities have different numbers of entries");
    return 0;
}

// compact the kept columns on the device (dst: where each group's go, ngroups + 1 entries), then copy only those to the
// caller's buffers (no intermediate host copies)
static int compact(const ConsJob& j, const ConsArgs& a, const std::vector<long long>& dst) {
    const size_t kept = static_cast<size_t>(dst.back());
    if (!kept) return 0;
    long long* d_dst; uint8_t* d_cc; uint8_t* d_cp; double* d_cl = nullptr;
    SL_TRY(upload("cons.dst", dst.data(), dst.size(), &d_dst, j.s));
    SL_TRY(scratch("cons.cc", kept, &d_cc));
    SL_TRY(scratch("cons.cp", kept, &d_cp));
    if (j.lerr) SL_TRY(scratch("cons.cl", kept, &d_cl));
    SL_TRY(launch_compact(a, d_dst, d_cc, d_cp, d_cl, j.s));
    SL_HIP(hipMemcpy(j.cons, d_cc, kept, hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(j.phred, d_cp, kept, hipMemcpyDeviceToHost));
    if (j.lerr) SL_HIP(hipMemcpy(j.lerr, d_cl, sizeof(double) * kept, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------
// Boundary columns: exact host-libm re-evaluation

struct ConsFixes {
    std::vector<long long> pos;   // index into the uncompacted layout
    std::vector<double> val;      // 4 per entry
    std::vector<int> grp;         // group of an entry k_consensus_qf made (-1: another kernel's)
    std::vector<int> gflag;       // CONS_QF_Q4: the groups k_consensus_qf handed over
};

static int read_fixes(const ConsArgs& a, int fixn, bool handed_over, ConsFixes& f) {
    f.pos.resize(static_cast<size_t>(fixn));
    f.val.resize(static_cast<size_t>(fixn) * 4);
    f.grp.resize(static_cast<size_t>(fixn));
    SL_HIP(hipMemcpy(f.pos.data(), a.fix_pos, sizeof(long long) * f.pos.size(), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(f.val.data(), a.fix_val, sizeof(double) * f.val.size(), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(f.grp.data(), a.fix_grp, sizeof(int) * f.grp.size(), hipMemcpyDeviceToHost));
    if (handed_over) {
        f.gflag.resize(static_cast<size_t>(a.ngroups));
        SL_HIP(hipMemcpy(f.gflag.data(), a.gflag, sizeof(int) * f.gflag.size(), hipMemcpyDeviceToHost));
    }
    return 0;
}

static char phred_char(double le) {
    const double q = std::min(std::round(-10 * le / std::log(10)), 93.0);
    return static_cast<char>(static_cast<int>(q) + 33);
}

static void apply_fixes(const ConsJob& j, const ConsFixes& f, const std::vector<long long>& dst) {
    const std::vector<int64_t>& out_off = j.rows.out_off;
    for (size_t k = 0; k < f.pos.size(); ++k) {
        // entries the fast kernel made for a group it later handed over are void (the generic kernel made its own)
        if (f.grp[k] >= 0 && !f.gflag.empty() && f.gflag[static_cast<size_t>(f.grp[k])]) continue;
        const double* v = &f.val[4 * k];
        const double le = j.quality ? log_error(v[0], v[1], v[2], v[3]) : std::log1p(-((v[0] + j.pseudo / 4) / (v[1] + j.pseudo)));
        // the entry's position is an index into the uncompacted layout: find its alignment, then its slot
        const long long pos = f.pos[k];
        const int64_t g = static_cast<int64_t>(std::upper_bound(out_off.begin(), out_off.begin() + j.ng_eval, pos) - out_off.begin()) - 1;
        const size_t at = static_cast<size_t>(dst[g] + (pos - out_off[g]));
        j.phred[at] = phred_char(le);
        if (j.lerr) j.lerr[at] = le;
    }
}

// ---------------------------------------------------------------------------
// Device part of the consensus: the job arrives with the alignment rows and (quality mode) the quality strings already
// in HBM; this adds the row table, the tables and scratch, launches the vote and resolves results and errors on the host.
static int consensus_core(const ConsJob& j) {
    Context& c = ctx();
    ConsShape shape;
    shape.quality = j.quality; shape.want_lerr = j.lerr != nullptr; shape.codes = j.a.codes != nullptr;
    shape.enc_n = j.enc_n; shape.qoffset = j.quality ? static_cast<int>(j.enc_names[0]) : 0;
    shape.opt_generic = option(OPT_CONSENSUS_GENERIC);   // (opt_chars had its say before the MSA stage: codes are present or not)
    shape.max_rows = j.rows.max_rows; shape.aln_bytes = j.rows.rel.back(); shape.qual_bytes = j.a.qual_bytes;
    shape.ng_eval = j.ng_eval; shape.num_cu = c.num_cu;
    const ConsPlan plan = cons_plan(shape);
    if (plan.refused) return fail("sarlacc_amd: alignment with %d rows does not fit the consensus kernel", j.rows.max_rows);

    ConsArgs a = j.a;
    a.ngroups = j.ng_eval;
    a.mincov = j.min_cov; a.pseudo = j.pseudo; a.ln10 = std::log(10);
    a.qoffset = shape.qoffset; a.navail = j.quality ? j.enc_n : 0;
    SL_TRY(upload_rows(j.rows, a, j.s));
    SL_TRY(upload_tables(cons_tables(j.enc_errors, j.enc_n, plan.route), a, j.s));
    SL_TRY(vote_scratch(j, a));
    if (j.ng_eval > 0) {
        SL_HIP(hipEventRecord(c.ev_start, j.s));
        c.counts["consensus_cells"] = static_cast<double>(j.total);
        c.counts["consensus_route"] = static_cast<double>(plan.route);
        c.counts["consensus_vote_passes"] = 1;
        c.stage_reset("consensus");
        SL_TRY(c.stage_begin("consensus", j.s));
        SL_TRY(launch_vote(plan, a, j.s));
        SL_HIP(hipEventRecord(c.ev_stop, j.s));
        SL_TRY(c.stage_end("consensus", j.s));
        c.timed = true;
    }
    ConsOutcome o;
    SL_TRY(read_back(j, a, o));
    SL_TRY(first_error(j, o));
    // More boundary columns than the list holds (every column of an alignment of equal rows can sit on one): the count
    // is exact and the kernels are deterministic, so the vote runs once more with a list of that size.
    while (o.fixn > a.fix_cap) {
        SL_TRY(fix_list(a, o.fixn, j.s));
        SL_TRY(launch_vote(plan, a, j.s));
        c.count_add("consensus_vote_passes", 1);
        SL_HIP(hipMemcpy(&o.fixn, a.fix_count, sizeof o.fixn, hipMemcpyDeviceToHost));
    }

    std::vector<long long> dst(static_cast<size_t>(j.ngroups) + 1, 0);
    for (int64_t g = 0; g < j.ngroups; ++g) dst[g + 1] = dst[g] + o.len[g];
    // (the caller's buffers hold the KEPT columns: their number is known only now -- the alignments of clusters of several
    // molecules are several reads wide and keep one read's worth of columns, so a bound from the widths would refuse, and make a
    // caller repeat, calls whose results fit easily)
    if (j.cons_cap >= 0 && dst.back() > j.cons_cap) return fail("sarlacc_amd: consensus output buffer too small (%lld needed)", dst.back());
    SL_TRY(compact(j, a, dst));
    if (o.fixn > 0) {
        ConsFixes f;
        SL_TRY(read_fixes(a, o.fixn, plan.route == CONS_QF_Q4, f));
        apply_fixes(j, f, dst);
    }
    for (int64_t g = 0; g < j.ngroups; ++g) j.cons_off[g + 1] = dst[g + 1];
    return 0;
}

// host-side structural checks, in the reference's order (group by group): equal row widths (src/DNA_input.cpp:90-104),
// then matching entry counts (:186-190).  group: the first one in error (-1: none).
struct ConsStructure { ConsStructErr err = CONS_STRUCT_OK; int64_t group = -1; };
static ConsStructure check_structure(bool quality, const int64_t* aln_off, const int64_t* grp_rows, const int64_t* qgrp_rows, int64_t ngroups) {
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t r0 = grp_rows[g], r1 = grp_rows[g + 1];
        for (int64_t r = r0 + 1; r < r1; ++r)
            if (aln_off[r + 1] - aln_off[r] != aln_off[r0 + 1] - aln_off[r0]) return {CONS_ROW_WIDTHS_DIFFER, g};
        if (quality && (qgrp_rows[g + 1] - qgrp_rows[g]) != (r1 - r0)) return {CONS_ENTRY_COUNTS_DIFFER, g};
    }
    return {};
}

static int run_consensus(bool quality, const char* aln, const int64_t* aln_off, const int64_t* grp_rows,
                         int64_t ngroups, const char* qual, const int64_t* qual_off, const int64_t* qgrp_rows,
                         double min_cov, double pseudo, const double* enc_errors, const char* enc_names, int enc_n,
                         char* cons, char* phred, int64_t* cons_off, double* lerr) {
    if (ngroups < 0) return fail("sarlacc_amd: negative number of alignments");
    if (quality) SL_TRY(check_encoding(enc_errors, enc_names, enc_n));
    cons_off[0] = 0;
    if (ngroups == 0) return 0;

    const ConsStructure st = check_structure(quality, aln_off, grp_rows, qgrp_rows, ngroups);
    ConsJob j;
    j.quality = quality;
    j.ngroups = ngroups;
    // Only groups before the first structural error are evaluated on the device.
    j.ng_eval = st.group >= 0 ? st.group : ngroups;
    j.rows_eval = grp_rows[j.ng_eval];
    j.struct_err = st.err;
    if (quality)
        for (int64_t g = 0; g < j.ng_eval; ++g)
            if (qgrp_rows[g] != grp_rows[g]) return fail("sarlacc_amd: alignment and quality row numbering differ");

    SL_TRY(ensure_device());
    const int64_t base = aln_off[0];
    j.total = aln_off[grp_rows[ngroups]] - base;
    j.rows = rows_from_offsets(aln_off, grp_rows, ngroups, st.group >= 0 ? st.group + 1 : ngroups);
    j.aln_host = aln + base;

    uint8_t* d_aln;
    SL_TRY(upload("cons.aln", reinterpret_cast<const uint8_t*>(aln) + base, static_cast<size_t>(j.total), &d_aln, j.s));
    j.a.aln = d_aln;
    if (quality) {
        const int64_t qrows = qgrp_rows[j.ng_eval];
        const int64_t qbase = qual_off[0];
        const int64_t qtotal = qual_off[qrows] - qbase;
        std::vector<int64_t> qrel(static_cast<size_t>(qrows) + 1);
        for (int64_t r = 0; r <= qrows; ++r) qrel[r] = qual_off[r] - qbase;
        uint8_t* d_q; int64_t* d_qoff;
        SL_TRY(upload("cons.qual", reinterpret_cast<const uint8_t*>(qual) + qbase, static_cast<size_t>(qtotal), &d_q, j.s));
        SL_TRY(upload("cons.qoff", qrel.data(), qrel.size(), &d_qoff, j.s));
        j.a.qual = d_q; j.a.qual_off = d_qoff; j.a.qual_bytes = qtotal;
    }
    j.min_cov = min_cov; j.pseudo = pseudo;
    j.enc_errors = enc_errors; j.enc_names = enc_names; j.enc_n = enc_n;
    j.cons = cons; j.phred = phred; j.cons_off = cons_off; j.lerr = lerr;
    return consensus_core(j);
}

// Shared body of sarlacc_msa_consensus (host pointers) and sarlacc_dev_msa_consensus (reads and
// qualities already in HBM: d_seq / d_qual non-null, seq / qual unused).
static int msa_consensus_impl(const int64_t* grp_off, const int32_t* grp, int64_t ngroups, const char* seq,
                              const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t nseq, double match,
                              double mismatch, double gap_extension, double gap_opening, int bandwidth, double min_cov,
                              double pseudo_count, const double* enc_errors, const char* enc_names, int enc_n, char* cons,
                              char* phred, int64_t* cons_off, int64_t cons_cap, const uint8_t* d_seq_res, const uint8_t* d_qual_res,
                              bool quality) {
    if (ngroups < 0 || nseq < 0) return fail("sarlacc_amd: negative sizes");
    if (quality) SL_TRY(check_encoding(enc_errors, enc_names, enc_n));
    cons_off[0] = 0;
    if (ngroups == 0) return 0;
    MsaResult res;
    res.width.assign(static_cast<size_t>(ngroups), 0);
    res.out_off.assign(static_cast<size_t>(ngroups) + 1, 0);
    // the quality strings travel to the device on a stream of their own while the pairwise
    // alignments run (qualities stay in read order; every row finds its string through the member list)
    uint8_t* d_q = nullptr; int64_t* d_qoff = nullptr;
    hipStream_t copy_stream = nullptr;
    hipEvent_t q_ready = nullptr;
    std::vector<int64_t> qrel;
    // Rows as vote codes (k_consensus_code) when the table allows it and the quality strings are laid out like the reads --
    // every read as long as its quality string, which is also what the reference demands; otherwise characters.
    ConsShape shape;
    shape.quality = quality; shape.enc_n = enc_n; shape.qoffset = quality ? static_cast<int>(enc_names[0]) : 0;
    shape.opt_chars = option(OPT_CONSENSUS_CHARS);
    bool codes = cons_codes_allowed(shape);
    for (int64_t r = 0; codes && r < nseq; ++r)
        if (qual_off[r + 1] - qual_off[r] != seq_off[r + 1] - seq_off[r]) codes = false;
    const uint8_t* d_q_const = nullptr;
    if (codes) {
        SL_TRY(ensure_device());
        int* d_bad;
        SL_TRY(scratch("cons.codebad", 1, &d_bad));
        const int none = INT_MAX;
        SL_HIP(hipMemcpy(d_bad, &none, sizeof none, hipMemcpyHostToDevice));
        SL_HIP(hipEventCreateWithFlags(&q_ready, hipEventDisableTiming));
        res.code.want = true; res.code.qual = &d_q_const; res.code.ready = q_ready;
        res.code.qoffset = shape.qoffset; res.code.navail = enc_n; res.code.d_bad = d_bad;
    }
    const std::function<int()> upload_quals = [&]() -> int {
        if (!quality) return 0;
        const int64_t qbase = qual_off[0];
        qrel.resize(static_cast<size_t>(nseq) + 1);
        for (int64_t r = 0; r <= nseq; ++r) qrel[r] = qual_off[r] - qbase;
        SL_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        if (d_qual_res) d_q = const_cast<uint8_t*>(d_qual_res);
        else SL_TRY(upload("cons.qual", reinterpret_cast<const uint8_t*>(qual) + qbase, static_cast<size_t>(qrel[nseq]), &d_q, copy_stream));
        SL_TRY(upload("cons.qoff", qrel.data(), qrel.size(), &d_qoff, copy_stream));
        d_q_const = d_q;
        if (q_ready) SL_HIP(hipEventRecord(q_ready, copy_stream));
        return 0;
    };
    struct EventGuard { hipEvent_t* e; ~EventGuard() { if (*e) (void)hipEventDestroy(*e); } } q_ready_guard{&q_ready};
    const int msa_rc = msa_run(grp_off, grp, ngroups, seq, seq_off, nseq, match, mismatch, gap_extension, gap_opening, bandwidth, true,
                               -1, &res, &upload_quals, d_seq_res);
    if (copy_stream) {
        const hipError_t e1 = hipStreamSynchronize(copy_stream), e2 = hipStreamDestroy(copy_stream);
        if (!msa_rc && (e1 != hipSuccess || e2 != hipSuccess)) return fail("HIP error while uploading the quality strings");
    }
    if (msa_rc) return msa_rc;
    if (quality && !d_q) return fail("sarlacc_amd: quality upload did not run");
    if (res.out_off[ngroups] == 0) {
        for (int64_t g = 0; g < ngroups; ++g) cons_off[g + 1] = 0;
        return 0;
    }
    ConsJob j;
    j.quality = quality;
    j.ngroups = j.ng_eval = ngroups;
    j.rows_eval = grp_off[ngroups] - grp_off[0];
    j.total = res.out_off[ngroups];
    j.rows = rows_from_widths(grp_off, res, ngroups);
    j.a.aln = res.d_out;
    if (codes) { j.a.codes = res.d_codes; j.a.code_bad = res.code.d_bad; }
    if (quality) { j.a.qual = d_q; j.a.qual_off = d_qoff; j.a.row_read = res.d_members; j.a.qual_bytes = qrel[static_cast<size_t>(nseq)]; }
    j.min_cov = min_cov; j.pseudo = pseudo_count;
    j.enc_errors = enc_errors; j.enc_names = enc_names; j.enc_n = enc_n;
    j.cons = cons; j.phred = phred; j.cons_off = cons_off; j.cons_cap = cons_cap;
    return consensus_core(j);
}

}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_create_consensus_basic_loop(const char* aln, const int64_t* aln_off, const int64_t* grp_rows,
                                        int64_t ngroups, double min_cov, double pseudo_count, char* cons,
                                        char* phred, int64_t* cons_off, double* lerr) {
    return run_consensus(false, aln, aln_off, grp_rows, ngroups, nullptr, nullptr, nullptr, min_cov, pseudo_count,
                         nullptr, nullptr, 0, cons, phred, cons_off, lerr);
}

int sarlacc_msa_consensus(const int64_t* grp_off, const int32_t* grp, int64_t ngroups, const char* seq,
                          const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t nseq, double match,
                          double mismatch, double gap_extension, double gap_opening, int bandwidth, double min_cov,
                          double pseudo_count, const double* enc_errors, const char* enc_names, int enc_n, char* cons,
                          char* phred, int64_t* cons_off, int64_t cons_cap) {
    return msa_consensus_impl(grp_off, grp, ngroups, seq, seq_off, qual, qual_off, nseq, match, mismatch, gap_extension,
                              gap_opening, bandwidth, min_cov, pseudo_count, enc_errors, enc_names, enc_n, cons, phred,
                              cons_off, cons_cap, nullptr, nullptr, qual != nullptr);
}

int sarlacc_dev_msa_consensus(const int64_t* grp_off, const int32_t* grp, int64_t ngroups, const uint8_t* d_seq,
                              const uint8_t* d_qual, const int64_t* off, int64_t nseq, double match, double mismatch,
                              double gap_extension, double gap_opening, int bandwidth, double min_cov, double pseudo_count,
                              const double* enc_errors, const char* enc_names, int enc_n, char* cons, char* phred,
                              int64_t* cons_off, int64_t cons_cap) {
    if (!d_seq) return fail("sarlacc_amd: sarlacc_dev_msa_consensus needs the reads in device memory");
    return msa_consensus_impl(grp_off, grp, ngroups, nullptr, off, nullptr, off, nseq, match, mismatch, gap_extension,
                              gap_opening, bandwidth, min_cov, pseudo_count, enc_errors, enc_names, enc_n, cons, phred,
                              cons_off, cons_cap, d_seq, d_qual, d_qual != nullptr);
}

int sarlacc_create_consensus_quality_loop(const char* aln, const int64_t* aln_off, const int64_t* grp_rows,
                                          int64_t ngroups, const char* qual, const int64_t* qual_off,
                                          const int64_t* qgrp_rows, double min_cov, const double* enc_errors,
                                          const char* enc_names, int enc_n, char* cons, char* phred,
                                          int64_t* cons_off, double* lerr) {
    return run_consensus(true, aln, aln_off, grp_rows, ngroups, qual, qual_off, qgrp_rows, min_cov, 0.0, enc_errors,
                         enc_names, enc_n, cons, phred, cons_off, lerr);
}
}
