// align_panel.hip -- barcodeAlign's loop over a panel of barcodes (R/barcodeAlign.R:20-37 around
// src/barcode_align.cpp:10-44) in one call: every barcode against a resident batch in global mode, and the best /
// next-best reduction on the device.
//
// k_barcode_panel is the fused path for barcodes of 1 to PANEL_COLS columns.  Mapping: ONE READ PER LANE, the barcode's
// columns unrolled in registers.
//   * The barcode is the same for the whole wavefront: its length and the table rows its columns read sit in SGPRs, all
//     control flow over columns is uniform, and nothing crosses lanes -- no skew, no DPP.
//   * Per column a lane keeps the score of the previous row and the vertical jump score in VGPRs (2 doubles per column).
//   * A read's (base, quality) pairs are staged once into LDS as byte offsets into a block of cost table rows (the layout
//     of build_cost_rows: one add per cell), PANEL_ROWS rows at a time; reads of up to PANEL_ROWS bases are staged once per
//     panel, longer ones once per barcode and chunk.
//   * The panel shares one cost table in LDS: the eight A/C/G/T rows plus the classes (2-fold, 3-fold, N) any barcode holds.
//   * A lane whose read has ended is masked; its column state stays what it was after its own last row.
// Every cell is the fp64 add / sub / compare sequence of the reference in its order (src/reference_align.cpp:54-181, as in
// k_align, whose argument for dropping the penalty selects when gapopen >= 0 holds here unchanged); the file is compiled
// with -ffp-contract=off, so a pair's score is the double sarlacc_barcode_align gives for it.
//
// Barcodes the kernel does not take (no columns, more than PANEL_COLS, a table that does not fit) go through run_align
// into a score row, which k_panel_fold folds into the running (barcode, score, next best).  The fold of
// R/barcodeAlign.R:27-35 depends on the order (strict comparisons: the first of equal scores wins), so the panel is walked
// in its order: maximal runs of consecutive fused barcodes are one launch each, with the running state kept in HBM.
#include "align_host.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <limits>

namespace sarlacc {

constexpr int PANEL_COLS = 32;    // columns of a barcode the fused kernel holds in registers
constexpr int PANEL_ROWS = 32;    // read positions staged per lane at a time
constexpr int PANEL_WAVES = 4;    // wavefronts per workgroup (they share the cost table)
constexpr size_t PANEL_LDS = 64 * 1024;

struct PanelArgs {
    const uint8_t* seq;
    const uint8_t* qual;
    const int64_t* off;
    long long n;
    int qoffset, navail, row_bytes;
    double GO, GE;
    const double* tables;        // build_cost_rows over the columns of every fused barcode
    int tab_doubles;
    const double* rowzero;       // [PANEL_COLS + 1] DP row 0: the same for every barcode
    int nb;                      // barcodes of this launch
    const int* bc_len;           // [nb]
    const int* bc_id;            // [nb] position in the panel, 0-based
    const uint32_t* bc_colbase;  // [nb][PANEL_COLS] byte offset (inside `tables`) of the rows a column reads
    int32_t* best;               // running state, read and written
    double* cur;
    double* next;
    double* all;                 // [nbarcodes][n] or null
};

typedef const double __attribute__((address_space(3))) lds_cdouble;

// R/barcodeAlign.R:27-35 for one read and one score
__device__ __forceinline__ void panel_fold(double s, int id1, int& id, double& cur, double& next) {
    if (s > cur) { next = cur; cur = s; id = id1; }
    else if (s > next) next = s;
}

// CAP: columns held in registers (a multiple of 4; the barcodes of the launch have at most CAP).
// PENSEL: select the gap penalty of every step explicitly (gapopen < 0), see k_align.
template <int CAP, bool PENSEL>
__global__ void __launch_bounds__(64 * PANEL_WAVES, CAP <= 8 ? 4 : (CAP <= 24 && !(PENSEL && CAP > 16)) ? 3 : 2) k_barcode_panel(const PanelArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int ENT_BYTES = PANEL_WAVES * PANEL_ROWS * 64 * static_cast<int>(sizeof(uint16_t));
    double* const s_tab = reinterpret_cast<double*>(smem + ENT_BYTES);
    const int lds_tab = static_cast<int>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)smem)) + ENT_BYTES;
    for (int x = threadIdx.x; x < A.tab_doubles; x += 64 * PANEL_WAVES) s_tab[x] = A.tables[x];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint16_t* const s_ent = reinterpret_cast<uint16_t*>(smem) + wave * (PANEL_ROWS * 64) + lane;   // [row][lane]
    const double NEG_INF = -__builtin_huge_val();
    const double GO = A.GO, GE = A.GE;

    const long long stride = static_cast<long long>(gridDim.x) * PANEL_WAVES * 64;
    for (long long base = (static_cast<long long>(blockIdx.x) * PANEL_WAVES + wave) * 64; base < A.n; base += stride) {
        const long long read = base + lane;
        const bool valid = read < A.n;
        const int L = valid ? static_cast<int>(A.off[read + 1] - A.off[read]) : 0;
        int m = L;
#pragma unroll
        for (int o = 32; o; o >>= 1) m = max(m, __shfl_xor(m, o));
        const int Lmax = __builtin_amdgcn_readfirstlane(m);
        const bool restage = Lmax > PANEL_ROWS;   // longer reads: every barcode stages its chunks again

        int id = 0;
        double cur = NEG_INF, next = NEG_INF;
        if (valid) { id = A.best[read]; cur = A.cur[read]; next = A.next[read]; }

        // rows [r0, r0 + PANEL_ROWS) of the lane's read as table offsets: (base code * navail + quality) * 8,
        // codes 0-3 = ACGT, 4 = anything else
        auto stage = [&](int r0) {
            const long long start = L > 0 ? A.off[read] : 0;   // (read again: not held in a register across the DP)
            for (int r = 0; r < PANEL_ROWS && r0 + r < Lmax; ++r) {
                if (r0 + r < L) {
                    const uint32_t b = A.seq[start + r0 + r];
                    int qi = static_cast<int>(static_cast<signed char>(A.qual[start + r0 + r])) - A.qoffset;
                    qi = qi < 0 ? 0 : (qi >= A.navail ? A.navail - 1 : qi);
                    const uint32_t code = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
                    s_ent[r * 64] = static_cast<uint16_t>(code * static_cast<uint32_t>(A.row_bytes) + static_cast<uint32_t>(qi << 3));
                }
            }
        };
        if (!restage) stage(0);

        for (int b = 0; b < A.nb; ++b) {
            const int R = A.bc_len[b];
            uint32_t cb[CAP];   // wave-uniform: the table rows of the barcode's columns
#pragma unroll
            for (int k = 0; k < CAP; ++k) cb[k] = A.bc_colbase[static_cast<size_t>(b) * PANEL_COLS + k];
            // per-column state: score of the previous row, vertical jump score; PENSEL: bit k of vmask = the move at
            // (previous row, column k) was a vertical gap
            double S[CAP], UJ[CAP];
#pragma unroll
            for (int k = 0; k < CAP; ++k) { S[k] = A.rowzero[k + 1]; UJ[k] = NEG_INF; }
            uint32_t vmask = 0;
            for (int r0 = 0; r0 < Lmax; r0 += PANEL_ROWS) {
                if (restage) stage(r0);
                const int rows = min(PANEL_ROWS, Lmax - r0);
                for (int r = 0; r < rows; ++r) {
                    const int i = r0 + r + 1;   // DP row
                    if (i <= L) {
                        const int ent = lds_tab + static_cast<int>(s_ent[r * 64]);
                        // column 0 (src/reference_align.cpp:63-78): rows i - 1 and i
                        double diag = i == 1 ? 0.0 : (-GO - GE * static_cast<double>(i - 2));
                        double left = -GO - GE * static_cast<double>(i - 1);
                        double lj = NEG_INF;
                        bool hp = false;   // PENSEL: the move at (row, previous column) was a horizontal gap
#pragma unroll
                        for (int k0 = 0; k0 < CAP; k0 += 4) {
                            // four columns per uniform branch; those past R compute values nothing reads (their table
                            // rows are column R's)
                            if (k0 < R) {
#pragma unroll
                                for (int k = k0; k < k0 + 4; ++k) {
                                    const double hcand = left - (PENSEL ? (hp ? GE : GO) : GO);
                                    const double ljm = lj - GE;
                                    const double H = fmax(ljm, hcand);
                                    lj = H;
                                    const double vcand = S[k] - (PENSEL ? (((vmask >> k) & 1u) ? GE : GO) : GO);
                                    const double ujm = UJ[k] - GE;
                                    const double V = fmax(ujm, vcand);
                                    UJ[k] = V;
                                    const double w = *reinterpret_cast<lds_cdouble*>(static_cast<uint32_t>(ent + static_cast<int>(cb[k])));
                                    const double M = diag + w;
                                    diag = S[k];
                                    // (:164-174): M only if greater than both, else H only if greater than V
                                    const double G = fmax(H, V);
                                    const double bestv = fmax(M, G);
                                    S[k] = bestv;
                                    left = bestv;
                                    if (PENSEL) {
                                        const bool b_hv = H > V, b_tm = M > G;
                                        hp = b_hv && !b_tm;
                                        const bool vn = !b_hv && !b_tm;
                                        vmask = (vmask & ~(1u << k)) | (vn ? (1u << k) : 0u);
                                    }
                                }
                            }
                        }
                    }
                }
            }
            // the score is the cell (L, R): column R's state after the lane's last row
            double sc = S[0];
#pragma unroll
            for (int k = 1; k < CAP; ++k) sc = (k == R - 1) ? S[k] : sc;
            const int pos = A.bc_id[b];
            panel_fold(sc, pos + 1, id, cur, next);
            if (A.all && valid) A.all[static_cast<size_t>(pos) * static_cast<size_t>(A.n) + static_cast<size_t>(read)] = sc;
        }
        if (valid) { A.best[read] = id; A.cur[read] = cur; A.next[read] = next; }
    }
}

// the state before the first barcode (R/barcodeAlign.R:20-22)
__global__ void k_panel_init(long long n, int32_t* best, double* cur, double* next) {
    const long long r = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (r >= n) return;
    best[r] = 0;
    cur[r] = -__builtin_huge_val();
    next[r] = -__builtin_huge_val();
}

// one barcode's score row into the running state
__global__ void k_panel_fold(long long n, const double* row, int id1, int32_t* best, double* cur, double* next) {
    const long long r = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (r >= n) return;
    int id = best[r];
    double c = cur[r], x = next[r];
    panel_fold(row[r], id1, id, c, x);
    best[r] = id;
    cur[r] = c;
    next[r] = x;
}

// What first_error (align_host.cpp) needs to know about the batch: out[0] the first read holding a quality below the encoding's
// first name, out[1] the first read that is not empty (INT_MAX: none).
__global__ void k_panel_scan(const uint8_t* qual, const int64_t* off, long long n, int qoffset, int* out) {
    const long long r = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (r >= n) return;
    const int64_t s = off[r], e = off[r + 1];
    if (e <= s) return;
    const int me = static_cast<int>(r);
    if (me < *const_cast<volatile int*>(out + 1)) atomicMin(out + 1, me);
    bool bad = false;
    for (int64_t p = s; p < e; ++p) bad = bad || static_cast<int>(static_cast<signed char>(qual[p])) < qoffset;
    if (bad) atomicMin(out, me);
}

// The error sarlacc_barcode_align raises for this barcode (first_error in align_host.cpp, which reads host offsets): inside an
// alignment column 1 is evaluated first -- its reference character, then the qualities of every row -- then the other columns.
static int panel_error(const char* ref, int R, int64_t len_bad, int64_t bad_qual_read, int64_t first_nonempty) {
    const int64_t INF = std::numeric_limits<int64_t>::max();
    int first_bad_col = -1;
    uint32_t tmp;
    for (int col = 0; col < R; ++col)
        if (column_info(ref[col], &tmp)) { first_bad_col = col; break; }
    const int64_t e_len = len_bad >= 0 ? len_bad : INF;
    const int64_t e_qual = R > 0 ? bad_qual_read : INF;
    const int64_t e_ref = first_bad_col >= 0 ? first_nonempty : INF;
    const int64_t first = std::min(e_len, std::min(e_qual, e_ref));
    if (first == INF) return 0;
    if (first == e_len) return fail("sequence and quality strings should have the same length");
    if (first == e_ref && first_bad_col == 0) return fail("unrecognized base in reference sequence");
    if (first == e_qual) return fail("quality cannot be lower than smallest encoded value");
    return fail("unrecognized base in reference sequence");
}

template <bool PENSEL>
static void launch_panel(int cap, const PanelArgs& a, int grid, size_t lds, hipStream_t s) {
    const dim3 g(static_cast<unsigned>(grid)), b(64 * PANEL_WAVES);
    if (cap <= 8) hipLaunchKernelGGL((k_barcode_panel<8, PENSEL>), g, b, lds, s, a);
    else if (cap <= 16) hipLaunchKernelGGL((k_barcode_panel<16, PENSEL>), g, b, lds, s, a);
    else if (cap <= 24) hipLaunchKernelGGL((k_barcode_panel<24, PENSEL>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_barcode_panel<32, PENSEL>), g, b, lds, s, a);
}

// The panel against a batch in HBM.  len_bad: the first read whose quality string has another length (host form; the
// batch's qualities were then not uploaded and only errors come out), else -1.
static int run_panel(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n, int32_t max_len,
                     const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                     const char* barcodes, const int64_t* barcode_off, int nbarcodes, int32_t* d_best, double* d_score,
                     double* d_next, double* d_all, hipStream_t stream, int64_t len_bad, int64_t host_first_nonempty) {
    Context& c = ctx();
    const int64_t INF = std::numeric_limits<int64_t>::max();
    const int IMAX = std::numeric_limits<int>::max();
    if (enc_n > 256) return fail("sarlacc_amd: encoding vector longer than 256 entries");
    if (n > IMAX - 8) return fail("sarlacc_amd: more than 2^31 reads in one call");
    const unsigned nblk = static_cast<unsigned>((n + 255) / 256);
    auto len_of = [&](int b) { return static_cast<int>(barcode_off[b + 1] - barcode_off[b]); };
    for (int b = 0; b < nbarcodes; ++b)
        if (barcode_off[b + 1] < barcode_off[b]) return fail("sarlacc_amd: barcode offsets should not decrease");

    // ---- the error the loop over the barcodes would raise first ----
    int64_t bad_qual = INF, first_nonempty = host_first_nonempty;
    if (len_bad < 0) {
        int* d_scan;
        const int none[2] = {IMAX, IMAX};
        int got[2] = {IMAX, IMAX};
        SL_TRY(upload("panel.scan", none, 2, &d_scan, stream));
        hipLaunchKernelGGL(k_panel_scan, dim3(nblk), dim3(256), 0, stream, d_qual, d_off, static_cast<long long>(n),
                           static_cast<int>(enc_names[0]), d_scan);
        SL_HIP(hipGetLastError());
        SL_HIP(hipMemcpyAsync(got, d_scan, sizeof got, hipMemcpyDeviceToHost, stream));
        SL_HIP(hipStreamSynchronize(stream));
        bad_qual = got[0] == IMAX ? INF : got[0];
        first_nonempty = got[1] == IMAX ? INF : got[1];
    }
    for (int b = 0; b < nbarcodes; ++b)
        SL_TRY(panel_error(barcodes + barcode_off[b], len_of(b), len_bad, bad_qual, first_nonempty));
    // (a batch with len_bad >= 0 gets here only with an empty panel: barcode 1 raises the length error or an earlier one)

    // ---- which barcodes the fused kernel takes, and their shared table ----
    const double GO = gapopen + gapext, GE = gapext;   // (src/reference_align.cpp:8)
    const bool pensel = !(GO >= GE) || option(OPT_ALIGN_PENSEL) != 0;
    std::vector<int> fused_len, fused_id;
    std::vector<uint32_t> colinfo(1, 0);   // 1-based, the columns of the fused barcodes one after the other
    if (option(OPT_ALIGN_PANEL) >= 0)
        for (int b = 0; b < nbarcodes; ++b) {
            const int R = len_of(b);
            if (R < 1 || R > PANEL_COLS) continue;
            fused_len.push_back(R);
            fused_id.push_back(b);
            for (int col = 0; col < R; ++col) {
                uint32_t info = 0;
                (void)column_info(barcodes[barcode_off[b] + col], &info);   // (valid: panel_error passed)
                colinfo.push_back(info);
            }
        }
    std::vector<double> tab, rows;
    std::vector<uint32_t> colbase;
    build_tables(enc_errors, enc_n, tab);
    build_cost_rows(tab, enc_n, colinfo.data(), static_cast<int>(colinfo.size()) - 1, rows, colbase);
    const size_t lds = sizeof(uint16_t) * PANEL_WAVES * PANEL_ROWS * 64 + sizeof(double) * rows.size();
    if (lds > PANEL_LDS) { fused_len.clear(); fused_id.clear(); }   // the table does not fit: every barcode on its own
    const int nfused = static_cast<int>(fused_len.size());

    PanelArgs a{};
    if (nfused) {
        std::vector<uint32_t> cbs(static_cast<size_t>(nfused) * PANEL_COLS);
        size_t at = 1;
        for (int f = 0; f < nfused; ++f) {
            for (int k = 0; k < PANEL_COLS; ++k) cbs[static_cast<size_t>(f) * PANEL_COLS + k] = colbase[at + std::min(k, fused_len[f] - 1)];
            at += fused_len[f];
        }
        double rowzero[PANEL_COLS + 1];
        rowzero[0] = 0.0;
        for (int col = 1; col <= PANEL_COLS; ++col) rowzero[col] = rowzero[col - 1] - (col == 1 ? GO : GE);   // (:115-118)
        double* d_tab; double* d_rz; int* d_len; int* d_id; uint32_t* d_cb;
        SL_TRY(upload("panel.tab", rows.data(), rows.size(), &d_tab, stream));
        SL_TRY(upload("panel.rz", rowzero, PANEL_COLS + 1, &d_rz, stream));
        SL_TRY(upload("panel.len", fused_len.data(), fused_len.size(), &d_len, stream));
        SL_TRY(upload("panel.id", fused_id.data(), fused_id.size(), &d_id, stream));
        SL_TRY(upload("panel.cb", cbs.data(), cbs.size(), &d_cb, stream));
        SL_HIP(hipStreamSynchronize(stream));   // the copies read this frame's vectors
        a.seq = d_seq; a.qual = d_qual; a.off = d_off; a.n = n;
        a.qoffset = static_cast<int>(enc_names[0]); a.navail = enc_n; a.row_bytes = static_cast<int>(enc_n * sizeof(double));
        a.GO = GO; a.GE = GE;
        a.tables = d_tab; a.tab_doubles = static_cast<int>(rows.size()); a.rowzero = d_rz;
        a.bc_len = d_len; a.bc_id = d_id; a.bc_colbase = d_cb;
        a.best = d_best; a.cur = d_score; a.next = d_next; a.all = d_all;
    }
    const long long nbatch = (n + 63) / 64;
    const int grid = static_cast<int>(align_grid(nbatch, PANEL_WAVES, c.num_cu));   // as run_align: far more workgroups than fit at once

    // ---- the panel in its order ----
    hipLaunchKernelGGL(k_panel_init, dim3(nblk), dim3(256), 0, stream, static_cast<long long>(n), d_best, d_score, d_next);
    SL_HIP(hipGetLastError());
    c.stage_reset("panel_dp");
    int launches = 0, singles = 0;
    double* d_row = nullptr;
    for (int b = 0, f = 0; b < nbarcodes;) {
        if (f < nfused && fused_id[f] == b) {
            int f1 = f + 1;   // the run of consecutive fused barcodes from b
            while (f1 < nfused && fused_id[f1] == fused_id[f1 - 1] + 1) ++f1;
            PanelArgs run = a;
            run.nb = f1 - f; run.bc_len = a.bc_len + f; run.bc_id = a.bc_id + f;
            run.bc_colbase = a.bc_colbase + static_cast<size_t>(f) * PANEL_COLS;
            const int cap = *std::max_element(fused_len.begin() + f, fused_len.begin() + f1);
            SL_TRY(c.stage_begin("panel_dp", stream));
            if (pensel) launch_panel<true>(cap, run, grid, lds, stream);
            else launch_panel<false>(cap, run, grid, lds, stream);
            SL_HIP(hipGetLastError());
            SL_TRY(c.stage_end("panel_dp", stream));
            ++launches;
            b += f1 - f;
            f = f1;
            continue;
        }
        AlignJob job{{d_seq, d_qual, d_off, n, max_len}, {enc_errors, enc_names, enc_n, gapopen, gapext}, barcodes + barcode_off[b], len_of(b), false, 0};
        job.stream = stream;
        AlignOut& out = job.out;
        if (d_all) out.d_scores = d_all + static_cast<size_t>(b) * static_cast<size_t>(n);
        else {
            if (!d_row) SL_TRY(scratch("panel.row", static_cast<size_t>(n), &d_row));
            out.d_scores = d_row;
        }
        int bad = 0;
        ChunkOpts co;
        co.stage = "panel_dp";
        SL_TRY(run_align(job, &bad, co));
        hipLaunchKernelGGL(k_panel_fold, dim3(nblk), dim3(256), 0, stream, static_cast<long long>(n), out.d_scores, b + 1, d_best,
                           d_score, d_next);
        SL_HIP(hipGetLastError());
        ++launches;
        ++singles;
        ++b;
    }
    SL_HIP(hipStreamSynchronize(stream));
    c.timed = Context::TIMED_PANEL;
    c.counts["panel_fused_barcodes"] = nfused;
    c.counts["panel_single_barcodes"] = singles;
    c.counts["panel_launches"] = launches;
    return 0;
}

}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_barcode_panel(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n, int32_t max_len,
                              const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                              const char* barcodes, const int64_t* barcode_off, int nbarcodes, int32_t* d_best,
                              double* d_score, double* d_next, double* d_all_scores, void* stream) {
    SL_TRY(check_encoding(enc_errors, enc_names, enc_n));
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    if (nbarcodes < 0) return fail("sarlacc_amd: negative number of barcodes");
    SL_TRY(ensure_device());
    if (n == 0) return 0;
    return run_panel(d_seq, d_qual, d_off, n, max_len, enc_errors, enc_names, enc_n, gapopen, gapext, barcodes, barcode_off,
                     nbarcodes, d_best, d_score, d_next, d_all_scores, static_cast<hipStream_t>(stream), -1, 0);
}

int sarlacc_barcode_panel(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                          const char* barcodes, const int64_t* barcode_off, int nbarcodes, int32_t* best, double* score,
                          double* next, double* all_scores) {
    SL_TRY(check_encoding(enc_errors, enc_names, enc_n));
    if (n < 0) return fail("sarlacc_amd: negative number of sequences");
    if (nbarcodes < 0) return fail("sarlacc_amd: negative number of barcodes");
    SL_TRY(ensure_device());
    if (n == 0) return 0;
    hipStream_t s = nullptr;
    HostBatch hb;
    SL_TRY(upload_batch(seq, seq_off, qual, qual_off, n, &hb, s));
    int64_t first_nonempty = std::numeric_limits<int64_t>::max();
    for (int64_t i = 0; i < n; ++i)
        if (seq_off[i + 1] - seq_off[i] > 0) { first_nonempty = i; break; }
    const size_t nn = static_cast<size_t>(n);
    int32_t* d_best; double* d_score; double* d_next; double* d_all = nullptr;
    SL_TRY(scratch("panel.best", nn, &d_best));
    SL_TRY(scratch("panel.score", nn, &d_score));
    SL_TRY(scratch("panel.next", nn, &d_next));
    if (all_scores && nbarcodes) SL_TRY(scratch("panel.all", nn * static_cast<size_t>(nbarcodes), &d_all));
    SL_TRY(run_panel(hb.d_seq, hb.d_qual, hb.d_off, n, hb.max_len, enc_errors, enc_names, enc_n, gapopen, gapext, barcodes,
                     barcode_off, nbarcodes, d_best, d_score, d_next, d_all, s, hb.len_bad, first_nonempty));
    SL_HIP(hipMemcpy(best, d_best, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(score, d_score, nn * sizeof(double), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(next, d_next, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (d_all) SL_HIP(hipMemcpy(all_scores, d_all, nn * static_cast<size_t>(nbarcodes) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
}
