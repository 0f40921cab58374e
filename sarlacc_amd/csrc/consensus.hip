// consensus.hip -- per-column consensus vote over per-group alignments on gfx950.
//
// Replaces internal_create_consensus_basic / _quality and their _loop wrappers
// (/root/reference/src/create_consensus.cpp:61-135, :178-272, :150-170, :287-308)
// and errorsToString (:18-32).
//
// Mapping: one wavefront per alignment (group); lanes own 64 consecutive columns,
// rows are streamed in the reference's row order so every per-column fp64 sum adds
// the same terms in the same order (bit-identical sums => identical base calls).
// The position of a base inside its ungapped quality string is a running prefix
// count of non-gap characters: per 64-column chunk it is ballot + popcount, the
// per-row carry sits in LDS.  Kept columns are compacted with the same trick.
// log1p(-e) / log(e/3) come from host-built tables (host libm); the device only
// evaluates transcendentals for the per-column error (log1p / exp), and columns
// whose Phred value falls within 1e-9 of a rounding boundary are re-evaluated on
// the host with the host libm so the emitted Phred characters never depend on
// device-vs-host libm differences.
//
// This is the one streaming, HBM-bound stage of the path: 2 B in per alignment
// cell (gapped base + quality), 2 B out per kept column.
//
// This file: the kernels and the two functions that launch them (at its end).  ConsArgs, the kernels' constants and the
// launch plan are in consensus.hpp; which kernels a call runs, its tables, scratch, results, errors and the C entry
// points are in consensus_host.cpp.
#include "consensus.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sarlacc {

// ascending sort of four scores (5 compare-exchanges)
__device__ __forceinline__ void sort4(double& a, double& b, double& c, double& d) {
    double t;
    if (a > b) { t = a; a = b; b = t; }
    if (c > d) { t = c; c = d; d = t; }
    if (a > c) { t = a; a = c; c = t; }
    if (b > d) { t = b; b = d; d = t; }
    if (b > c) { t = b; b = c; c = t; }
}

// append a column whose Phred value lies within 1e-9 of a rounding boundary to the list the host re-evaluates;
// GRP: also record its group (k_consensus_qf).  The list's fields come as arguments: a helper that reads them from
// the kernel's ConsArgs changes the code the compiler makes around it.
template <bool GRP = false>
__device__ __forceinline__ void push_fix(int* count, int cap, long long* fpos, double* fval, int* fgrp, long long pos, double a,
                                         double b, double c, double d, int grp = 0) {
    const int slot = atomicAdd(count, 1);
    if (slot < cap) {
        fpos[slot] = pos;
        if (GRP) fgrp[slot] = grp;
        fval[4 * slot + 0] = a; fval[4 * slot + 1] = b;
        fval[4 * slot + 2] = c; fval[4 * slot + 3] = d;
    }
}

template <bool QUALITY>
__global__ void __launch_bounds__(64) k_consensus(const ConsArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* s_right = reinterpret_cast<double*>(smem);
    double* s_wrong = s_right + (QUALITY ? A.navail : 0);
    long long* s_roff = reinterpret_cast<long long*>(s_wrong + (QUALITY ? A.navail : 0));
    long long* s_qoff = s_roff + A.max_rows;
    int* s_pos = reinterpret_cast<int*>(s_qoff + A.max_rows);
    int* s_bad = s_pos + A.max_rows;
    int* s_qlen = s_bad + A.max_rows;
    constexpr int RB = 8;

    const int lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (QUALITY)
        for (int x = lane; x < A.navail; x += 64) { s_right[x] = A.right[x]; s_wrong[x] = A.wrong[x]; }
    __syncthreads();

    for (long long g = blockIdx.x; g < A.ngroups; g += gridDim.x) {
        const long long row0 = A.grp_rows[g];
        const int nrows = static_cast<int>(A.grp_rows[g + 1] - row0);
        if (nrows == 0) {
            if (lane == 0) A.cons_len[g] = 0;
            continue;
        }
        const long long W = A.aln_off[row0 + 1] - A.aln_off[row0];
        const double thresh = static_cast<double>(nrows) * A.mincov;
        const long long obase = A.out_off[g];
        // per-row offsets once per group: no dependent scalar loads inside the column loop
        for (int r = lane; r < nrows; r += 64) {
            s_pos[r] = 0;
            s_bad[r] = 0;
            s_roff[r] = A.aln_off[row0 + r];
            if (QUALITY) {
                const long long q = A.row_read ? A.row_read[row0 + r] - 1 : row0 + r;
                s_qoff[r] = A.qual_off[q];
                s_qlen[r] = static_cast<int>(A.qual_off[q + 1] - A.qual_off[q]);
            }
        }
        __syncthreads();
        int outpos = 0;

        for (long long c0 = 0; c0 < W; c0 += 64) {
            const long long col = c0 + lane;
            const bool active = col < W;
            double sA = 0, sC = 0, sG = 0, sT = 0;
            int inc = 0;
            // rows in batches of RB: all alignment bytes of a batch are requested before any is
            // used, then all quality bytes -- two memory round trips per batch instead of per row.
            // Accumulation stays in row order, so the fp64 sums are the reference's.
            for (int r0 = 0; r0 < nrows; r0 += RB) {
                uint8_t ch[RB];
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    const int r = r0 + b;
                    ch[b] = (active && r < nrows) ? A.aln[s_roff[r < nrows ? r : 0] + col] : static_cast<uint8_t>('-');
                }
                int pq[RB];
                uint8_t qv8[RB];
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    const int r = r0 + b;
                    const bool nongap = ch[b] != '-';
                    const unsigned long long mask = __ballot(nongap);
                    pq[b] = -1;
                    if (QUALITY && r < nrows) {
                        const int p = s_pos[r] + __popcll(mask & lt);
                        if (lane == 0) s_pos[r] += __popcll(mask);
                        if (nongap && ch[b] != 'N' && p < s_qlen[r]) pq[b] = p;
                    }
                }
                if (QUALITY) {
#pragma unroll
                    for (int b = 0; b < RB; ++b) {
                        const int r = r0 + b;
                        qv8[b] = (pq[b] >= 0) ? A.qual[s_qoff[r < nrows ? r : 0] + pq[b]] : static_cast<uint8_t>(0);
                    }
                }
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    const int r = r0 + b;
                    const uint8_t c = ch[b];
                    if (c == '-') continue;
                    ++inc;
                    if (QUALITY) {
                        if (pq[b] >= 0) {
                            int qi = static_cast<int>(static_cast<signed char>(qv8[b])) - A.qoffset;
                            if (qi < 0) { s_bad[r] = 1; qi = 0; }
                            if (qi >= A.navail) qi = A.navail - 1;
                            const double right = s_right[qi], wrong = s_wrong[qi];
                            sA += (c == 'A') ? right : wrong;
                            sC += (c == 'C') ? right : wrong;
                            sG += (c == 'G') ? right : wrong;
                            sT += (c == 'T') ? right : wrong;
                        }
                    } else if (c != 'N') {
                        if (c == 'A') sA += 1;
                        else if (c == 'C') sC += 1;
                        else if (c == 'G') sG += 1;
                        else if (c == 'T') sT += 1;
                        else atomicMin(A.first_bad_char, static_cast<unsigned long long>(s_roff[r] + col));
                    }
                }
            }
            const bool keep = active && !(inc < thresh);
            // first maximum in A,C,G,T order (std::max_element)
            int best = 0;
            double bv = sA;
            if (sC > bv) { bv = sC; best = 1; }
            if (sG > bv) { bv = sG; best = 2; }
            if (sT > bv) { bv = sT; best = 3; }
            double le;
            double f0, f1, f2 = 0, f3 = 0;
            if (QUALITY) {
                double a = sA, b = sC, c = sG, d = sT;
                sort4(a, b, c, d);
                le = log_error(a, b, c, d);
                f0 = a; f1 = b; f2 = c; f3 = d;
            } else {
                int total = 0;
                total = static_cast<int>(total + sA);
                total = static_cast<int>(total + sC);
                total = static_cast<int>(total + sG);
                total = static_cast<int>(total + sT);
                const double p = (bv + A.pseudo / 4) / (static_cast<double>(total) + A.pseudo);
                le = log1p(-p);
                f0 = bv; f1 = static_cast<double>(total);
            }
            const double x = -10 * le / A.ln10;
            double qv = round(x);
            if (qv > 93.0) qv = 93.0;
            const double frac = x - floor(x);
            const bool near = keep && x < 93.4 && fabs(frac - 0.5) < 1e-9;

            const unsigned long long kmask = __ballot(keep);
            const int o = outpos + __popcll(kmask & lt);
            if (keep) {
                A.cons[obase + o] = "ACGT"[best];
                A.phred[obase + o] = static_cast<uint8_t>(static_cast<int>(qv) + 33);
                if (A.lerr) A.lerr[obase + o] = le;
                if (near) push_fix(A.fix_count, A.fix_cap, A.fix_pos, A.fix_val, A.fix_grp, obase + o, f0, f1, f2, f3);
            }
            outpos += __popcll(kmask);
        }
        if (lane == 0) A.cons_len[g] = outpos;
        if (QUALITY) {
            for (int r = lane; r < nrows; r += 64) {
                const int qlen = s_qlen[r];
                const int used = s_pos[r];
                A.row_status[row0 + r] = s_bad[r] ? 1 : (used == qlen ? 0 : (used > qlen ? 2 : 3));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// k_consensus_q4: the quality-weighted vote with 4 columns per lane.
//
// Same arithmetic as k_consensus<true> (rows in order, so every per-column fp64 sum adds the
// reference's terms in the reference's order) but laid out for bandwidth: a wavefront covers
// 256 columns per step, a lane reads its 4 alignment characters of a row with one (unaligned)
// dword load and, because the non-gap characters of a lane are consecutive in the ungapped
// quality string, their qualities with one more; rows are fetched in batches so several loads
// are in flight.  The (character, quality) -> four additions map is a table of 32-byte vectors
// in LDS shared by the 4 wavefronts of a workgroup (two ds_read_b128 + four v_add_f64 per cell;
// gaps, N and out-of-range positions read a zero vector, which leaves the sums bit-identical).
// The per-column error needs three log1pexp: they are first evaluated with the hardware fp32
// exp/log (absolute error < 1e-5 in the log-error), which decides the Phred character unless
// the value lies within 2e-4 of a rounding boundary; only those columns take the fp64 path,
// and columns within 1e-9 of a boundary go to the host libm as before.
typedef uint32_t __attribute__((aligned(1))) cons_u32_unaligned;

// exact fp64 log error of a column from its four sorted scores (out of line: rare, register-hungry)
__device__ __noinline__ double exact_log_error(double a, double b, double c, double d) { return log_error(a, b, c, d); }

__device__ __forceinline__ double fast_log1pexp(double x) {
    if (x > 33.3) return x;
    if (x > 18.) return x + static_cast<double>(__expf(static_cast<float>(-x)));
    const float y = __expf(static_cast<float>(x));
    return static_cast<double>(__logf(1.0f + y));
}

__global__ void __launch_bounds__(256, 4) k_consensus_q4(const ConsArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nvec = 5 * A.navail + 1;
    double* const s_vec = reinterpret_cast<double*>(smem);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long* const s_roff = reinterpret_cast<long long*>(s_vec + 4 * nvec) + wave * 2 * A.max_rows;
    long long* const s_qoff = s_roff + A.max_rows;
    int* const s_int = reinterpret_cast<int*>(reinterpret_cast<long long*>(s_vec + 4 * nvec) + 4 * 2 * A.max_rows) + wave * 3 * A.max_rows;
    int* const s_qlen = s_int;
    int* const s_pos = s_int + A.max_rows;
    int* const s_bad = s_int + 2 * A.max_rows;
    for (int x = threadIdx.x; x < 4 * nvec; x += 256) s_vec[x] = A.vec[x];
    __syncthreads();
    const int zero_entry = 5 * A.navail;

    for (long long g = static_cast<long long>(blockIdx.x) * 4 + wave; g < A.ngroups; g += static_cast<long long>(gridDim.x) * 4) {
        if (A.only_flagged && !A.gflag[g]) continue;
        const long long row0 = A.grp_rows[g];
        const int nrows = static_cast<int>(A.grp_rows[g + 1] - row0);
        if (nrows == 0) {
            if (lane == 0) A.cons_len[g] = 0;
            continue;
        }
        const long long W = A.aln_off[row0 + 1] - A.aln_off[row0];
        const double thresh = static_cast<double>(nrows) * A.mincov;
        const long long obase = A.out_off[g];
        for (int r = lane; r < nrows; r += 64) {
            s_pos[r] = 0;
            s_bad[r] = 0;
            s_roff[r] = A.aln_off[row0 + r];
            const long long q = A.row_read ? A.row_read[row0 + r] - 1 : row0 + r;
            s_qoff[r] = A.qual_off[q];
            s_qlen[r] = static_cast<int>(A.qual_off[q + 1] - A.qual_off[q]);
        }
        int outpos = 0;

        for (long long c0 = 0; c0 < W; c0 += 256) {
            const long long col = c0 + 4 * lane;
            const long long remain = W - col;          // characters of the row at and after `col`
            double acc[4][4];
            int inc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { inc[k] = 0; acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0; }

            for (int r0 = 0; r0 < nrows; r0 += Q4_RB) {
                uint32_t aw[Q4_RB], qw[Q4_RB];
                int pq[Q4_RB];
#pragma unroll
                for (int b = 0; b < Q4_RB; ++b) {
                    const int r = r0 + b;
                    uint32_t v = 0x2d2d2d2du;   // "----"
                    if (r < nrows && remain > 0) {
                        const uint8_t* src = A.aln + s_roff[r] + col;
                        if (remain >= 4) v = *reinterpret_cast<const cons_u32_unaligned*>(src);
                        else
                            for (int k = 0; k < remain; ++k) v = (v & ~(0xffu << (8 * k))) | (static_cast<uint32_t>(src[k]) << (8 * k));
                    }
                    aw[b] = v;
                }
#pragma unroll
                for (int b = 0; b < Q4_RB; ++b) {
                    const int r = r0 + b;
                    // position of this lane's first non-gap character in the row's ungapped string
                    int below = 0, total = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned long long m = __ballot(((aw[b] >> (8 * k)) & 0xffu) != 0x2du);
                        below += __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0));
                        total += __popcll(m);
                    }
                    pq[b] = 0;
                    if (r < nrows) {
                        pq[b] = s_pos[r] + below;
                        if (lane == 0) s_pos[r] += total;
                    }
                }
#pragma unroll
                for (int b = 0; b < Q4_RB; ++b) {
                    const int r = r0 + b;
                    uint32_t v = 0;
                    if (r < nrows) {
                        const int avail = s_qlen[r] - pq[b];
                        if (avail > 0) {
                            const uint8_t* src = A.qual + s_qoff[r] + pq[b];
                            if (avail >= 4) v = *reinterpret_cast<const cons_u32_unaligned*>(src);
                            else
                                for (int k = 0; k < avail; ++k) v |= static_cast<uint32_t>(src[k]) << (8 * k);
                        }
                    }
                    qw[b] = v;
                }
#pragma unroll
                for (int b = 0; b < Q4_RB; ++b) {
                    const int r = r0 + b;
                    if (r >= nrows) break;
                    const int avail = s_qlen[r] - pq[b];
                    int jq = 0;   // non-gap characters of this lane seen so far
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t c = (aw[b] >> (8 * k)) & 0xffu;
                        int entry = zero_entry;
                        if (c != 0x2du) {
                            ++inc[k];
                            if (c != 'N' && jq < avail) {
                                int qi = static_cast<int>(static_cast<signed char>((qw[b] >> (8 * jq)) & 0xffu)) - A.qoffset;
                                if (qi < 0) { s_bad[r] = 1; qi = 0; }
                                if (qi >= A.navail) qi = A.navail - 1;
                                const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
                                entry = code * A.navail + qi;
                            }
                            ++jq;
                        }
                        const double* vp = s_vec + 4 * entry;
                        acc[k][0] += vp[0]; acc[k][1] += vp[1]; acc[k][2] += vp[2]; acc[k][3] += vp[3];
                    }
                }
            }

            // ---- per-column result ----
            int nkept = 0;
            int below_kept = 0;
            bool keepk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                keepk[k] = (k < remain) && !(inc[k] < thresh);
                const unsigned long long m = __ballot(keepk[k]);
                below_kept += __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0));
                nkept += __popcll(m);
            }
            int o = outpos + below_kept;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!keepk[k]) continue;
                const double sA = acc[k][0], sC = acc[k][1], sG = acc[k][2], sT = acc[k][3];
                int best = 0;
                double bv = sA;
                if (sC > bv) { bv = sC; best = 1; }
                if (sG > bv) { bv = sG; best = 2; }
                if (sT > bv) { bv = sT; best = 3; }
                double a = sA, b = sC, c = sG, d = sT;
                sort4(a, b, c, d);
                double denom = a;
                denom += fast_log1pexp(b - denom);
                denom += fast_log1pexp(c - denom);
                double err3 = denom;
                denom += fast_log1pexp(d - denom);
                double le = err3 - denom;
                double x = -10 * le / A.ln10;
                double frac = x - floor(x);
                bool near = false;
                if (x < 93.4 && fabs(frac - 0.5) < 2e-4) {   // too close for the fp32 estimate: exact fp64 evaluation
                    le = exact_log_error(a, b, c, d);
                    x = -10 * le / A.ln10;
                    frac = x - floor(x);
                    near = x < 93.4 && fabs(frac - 0.5) < 1e-9;
                }
                double qv = round(x);
                if (qv > 93.0) qv = 93.0;
                A.cons[obase + o] = "ACGT"[best];
                A.phred[obase + o] = static_cast<uint8_t>(static_cast<int>(qv) + 33);
                if (near) push_fix(A.fix_count, A.fix_cap, A.fix_pos, A.fix_val, A.fix_grp, obase + o, a, b, c, d);
                ++o;
            }
            outpos += nkept;
        }
        if (lane == 0) A.cons_len[g] = outpos;
        for (int r = lane; r < nrows; r += 64) {
            const int qlen = s_qlen[r];
            const int used = s_pos[r];
            A.row_status[row0 + r] = s_bad[r] ? 1 : (used == qlen ? 0 : (used > qlen ? 2 : 3));
        }
    }
}

// ---------------------------------------------------------------------------
// k_consensus_qf: the quality vote on clean data, built around the instruction count per cell.
//
// Same sums in the same order as k_consensus_q4 (4 columns per lane, rows in order).  What is different:
//  * everything that can be done on the four characters of a lane at once is done on the dword: gap
//    detection, non-gap count, the position of every character in the quality string (byte-wise prefix
//    by one multiplication), the expansion of the lane's quality bytes to the slots of its characters
//    (one v_perm), range and alphabet checks;
//  * the wave prefix of the non-gap counts is one DPP scan for three rows (10-bit fields);
//  * the four addends of a cell come from LDS with ONE address: per quality value the table holds the
//    strip (w w w r w w w) of log(e/3) and log1p(-e); a cell of base code c reads strip[3 - c + b] for
//    base b = 0..3, i.e. four ds_read_b64 at immediate offsets from (row of q) + (3 - c) -- no select.
//    Base codes are (char >> 1) & 3: A 0, C 1, T 2, G 3.  Every double is replicated for 16 lane slots.
//    Gaps read the all-zero row (adding +0.0 leaves the sums bit-identical).
// It handles alignments of A, C, G, T and '-' with qualities inside the encoding, at most 64 rows stored
// back to back; anything else (N or other characters, a quality outside the table, quality strings
// shorter or longer than their rows, the last bytes of a buffer) sets the group's flag and the group is
// redone by k_consensus_q4 -- detection costs a few SWAR operations per dword and is exact.

// The results of the kept columns of a lane in k_consensus_qf / k_consensus_code (accumulators in code order A, C, T, G),
// written from output position obase + o on: the first maximum in the order A, C, G, T (std::max_element) and the
// Phred character.  The Phred value is estimated in fp32: with u = score - max, S = sum of exp(u) over the three other
// bases, the log error is log(S / (1 + S)) and the Phred value 10 log10(2) (log2(1 + S) - log2(S)).  Mathematically
// the value of the reference's log1pexp chain; the fp32 error (< 1e-4 in the Phred value) only matters next to a
// rounding boundary, where the exact chain is evaluated instead.  GRP: boundary entries record group g.
// (One helper for the whole loop: a helper per column makes the compiler lay out the stores differently.)
template <bool GRP>
__device__ __forceinline__ void emit_columns(const ConsArgs& A, const double (&acc)[4][4], const bool (&keepk)[4], long long obase, int o,
                                             long long g) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!keepk[k]) continue;
        const double sA = acc[k][0], sC = acc[k][1], sG = acc[k][3], sT = acc[k][2];
        const double mx = fmax(fmax(sA, sC), fmax(sG, sT));
        const int best = sA == mx ? 0 : (sC == mx ? 1 : (sG == mx ? 2 : 3));
        const float NEG = -1.0e30f;
        const float uA = best == 0 ? NEG : static_cast<float>(sA - mx), uC = best == 1 ? NEG : static_cast<float>(sC - mx);
        const float uG = best == 2 ? NEG : static_cast<float>(sG - mx), uT = best == 3 ? NEG : static_cast<float>(sT - mx);
        const float L2E = 1.44269504088896341f;
        const float S = (__builtin_amdgcn_exp2f(uA * L2E) + __builtin_amdgcn_exp2f(uC * L2E)) +
                        (__builtin_amdgcn_exp2f(uG * L2E) + __builtin_amdgcn_exp2f(uT * L2E));
        float xf = 3.01029995663981195f * (__builtin_amdgcn_logf(1.0f + S) - __builtin_amdgcn_logf(S));   // v_log_f32 = log2
        const float fr = xf - floorf(xf);
        int qv;
        bool near = false;
        double a = 0, b = 0, c = 0, d = 0;
        if (xf < 93.4f && fabsf(fr - 0.5f) < 4e-4f) {     // too close for the estimate: the reference's chain in fp64
            a = sA; b = sC; c = sG; d = sT;
            sort4(a, b, c, d);
            const double le = exact_log_error(a, b, c, d);
            const double x = -10 * le / A.ln10;
            const double frac = x - floor(x);
            near = x < 93.4 && fabs(frac - 0.5) < 1e-9;
            double q = round(x);
            if (q > 93.0) q = 93.0;
            qv = static_cast<int>(q);
        } else {
            xf = fminf(xf, 93.0f);                          // also takes +inf (S underflowed to 0)
            qv = static_cast<int>(floorf(xf + 0.5f));
        }
        A.cons[obase + o] = "ACGT"[best];
        A.phred[obase + o] = static_cast<uint8_t>(qv + 33);
        if (near) push_fix<GRP>(A.fix_count, A.fix_cap, A.fix_pos, A.fix_val, A.fix_grp, obase + o, a, b, c, d, static_cast<int>(g));
        ++o;
    }
}

__device__ __forceinline__ unsigned qf_scan(unsigned x) {   // inclusive prefix sum over the wavefront
    x += static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x111, 0xf, 0xf, false));   // row_shr:1
    x += static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x112, 0xf, 0xf, false));   // row_shr:2
    x += static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x114, 0xf, 0xf, false));   // row_shr:4
    x += static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x118, 0xf, 0xf, false));   // row_shr:8
    x += static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x142, 0xa, 0xf, false));   // row_bcast:15
    x += static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x143, 0xc, 0xf, false));   // row_bcast:31
    return x;
}

__global__ void __launch_bounds__(QF_THREADS) k_consensus_qf(const ConsArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    {
        const uint4* src = reinterpret_cast<const uint4*>(A.strip);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        const int n16 = (A.navail + 1) * (QF_ROWB / 16);
        for (int x = threadIdx.x; x < n16; x += QF_THREADS) dst[x] = src[x];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char* const lanebase = smem + (lane & 15) * 8;
    const unsigned DASH4 = 0x2d2d2d2du;
    const unsigned QOFF4 = static_cast<unsigned>(A.qoffset) * 0x01010101u;
    const unsigned QZERO4 = static_cast<unsigned>(A.qoffset + A.navail) * 0x01010101u;   // the quality "character" of the zero row
    const unsigned KHI = static_cast<unsigned>(0x80 - A.navail) * 0x01010101u;           // q + KHI has bit 7 set iff q >= navail
    const unsigned LUT = 0x47544341u;                                                    // code -> character: A C T G

    for (long long g = static_cast<long long>(blockIdx.x) * (QF_THREADS / 64) + wave; g < A.ngroups;
         g += static_cast<long long>(gridDim.x) * (QF_THREADS / 64)) {
        const long long row0 = A.grp_rows[g];
        const int nrows = static_cast<int>(A.grp_rows[g + 1] - row0);
        if (nrows == 0) {
            if (lane == 0) { A.cons_len[g] = 0; A.gflag[g] = 0; }
            continue;
        }
        const long long abase = A.aln_off[row0];
        const long long W = A.aln_off[row0 + 1] - abase;
        // row descriptors: lane r holds row r
        long long qo = 0;
        int qlen = 0;
        bool rowbad = false;
        if (lane < nrows && nrows <= 64) {
            const long long q = A.row_read ? A.row_read[row0 + lane] - 1 : row0 + lane;
            qo = A.qual_off[q];
            qlen = static_cast<int>(A.qual_off[q + 1] - qo);
            rowbad = A.aln_off[row0 + lane] != abase + static_cast<long long>(lane) * W || qo + qlen + 4 > A.qual_bytes;
        }
        if (nrows > 64 || W >= (1ll << 30) || abase + static_cast<long long>(nrows) * W + 4 > A.aln_bytes || __ballot(rowbad)) {
            if (lane == 0) A.gflag[g] = 1;
            continue;
        }
        const int qo_lo = static_cast<int>(qo), qo_hi = static_cast<int>(qo >> 32);
        int vpos = 0;
        unsigned bad = 0;
        const double thresh = static_cast<double>(nrows) * A.mincov;
        const long long obase = A.out_off[g];
        int outpos = 0;

        unsigned vn[QF_RB];
#pragma unroll
        for (int b = 0; b < QF_RB; ++b) {
            unsigned w = DASH4;
            if (b < nrows && 4 * lane < static_cast<int>(W)) w = *reinterpret_cast<const cons_u32_unaligned*>(A.aln + abase + static_cast<long long>(b) * W + 4 * lane);
            vn[b] = w;
        }
        for (long long c0 = 0; c0 < W; c0 += 256) {
            const int col = static_cast<int>(c0) + 4 * lane;
            const int remain = static_cast<int>(W) - col;          // characters of the row at and after `col`
            const unsigned keepmask = remain >= 4 ? 0xffffffffu : (remain <= 0 ? 0u : ((1u << (8 * remain)) - 1u));
            double acc[4][4];
            unsigned inc4 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;

            for (int r0 = 0; r0 < nrows; r0 += QF_RB) {
                unsigned v[QF_RB], ng[QF_RB], qw[QF_RB];
#pragma unroll
                for (int b = 0; b < QF_RB; ++b) v[b] = (vn[b] & keepmask) | (DASH4 & ~keepmask);   // requested one batch ahead
                unsigned pk[2] = {0u, 0u};
#pragma unroll
                for (int b = 0; b < QF_RB; ++b) {
                    const unsigned x = v[b] ^ DASH4;
                    const unsigned t = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
                    ng[b] = t & 0x80808080u;                        // bit 7 of every non-gap byte
                    pk[b / 3] |= static_cast<unsigned>(__builtin_popcount(ng[b])) << (10 * (b % 3));
                }
                const unsigned sc0 = qf_scan(pk[0]), sc1 = qf_scan(pk[1]);
                const unsigned tot0 = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(sc0), 63));
                const unsigned tot1 = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(sc1), 63));
#pragma unroll
                for (int b = 0; b < QF_RB; ++b) {
                    const int r = r0 + b;
                    const int rr = r < 63 ? r : 63;
                    const unsigned incl = ((b < 3 ? sc0 : sc1) >> (10 * (b % 3))) & 0x3ffu;
                    const unsigned total = ((b < 3 ? tot0 : tot1) >> (10 * (b % 3))) & 0x3ffu;
                    const int n = __builtin_popcount(ng[b]);
                    const int carry = __builtin_amdgcn_readlane(vpos, rr);
                    const int ql = __builtin_amdgcn_readlane(qlen, rr);
                    const int pos = carry + static_cast<int>(incl) - n;
                    if (r < nrows && lane == rr) vpos = carry + static_cast<int>(total);
                    bad |= (r < nrows && pos + n > ql) ? 0x80u : 0u;
                    unsigned w = QZERO4;
                    if (r < nrows && n > 0) {
                        const long long qb = (static_cast<long long>(__builtin_amdgcn_readlane(qo_hi, rr)) << 32) |
                                             static_cast<unsigned>(__builtin_amdgcn_readlane(qo_lo, rr));
                        w = *reinterpret_cast<const cons_u32_unaligned*>(A.qual + qb + (pos < ql ? pos : ql));
                    }
                    qw[b] = w;
                }
                {   // characters of the next batch (next rows of this step, or the first rows of the next step)
                    const bool wrap = r0 + QF_RB >= nrows;
                    const int nr0 = wrap ? 0 : r0 + QF_RB;
                    const int ncol = wrap ? col + 256 : col;
#pragma unroll
                    for (int b = 0; b < QF_RB; ++b) {
                        const int r = nr0 + b;
                        unsigned w = DASH4;
                        if (r < nrows && ncol < static_cast<int>(W)) w = *reinterpret_cast<const cons_u32_unaligned*>(A.aln + abase + static_cast<long long>(r) * W + ncol);
                        vn[b] = w;
                    }
                }
#pragma unroll
                for (int b = 0; b < QF_RB; ++b) {
                    if (r0 + b >= nrows) break;
                    const unsigned one = ng[b] >> 7;                                     // 1 per non-gap byte
                    const unsigned ff = (ng[b] << 1) - one;                              // 0xff per non-gap byte
                    const unsigned presel = (one << 8) + (one << 16) + (one << 24);      // byte k: non-gap bytes below k
                    const unsigned sel = (presel & ff) | (0x04040404u & ~ff);
                    const unsigned qe = __builtin_amdgcn_perm(QZERO4, qw[b], sel);       // quality of every character, zero row for gaps
                    const unsigned qi = qe - QOFF4;
                    bad |= (qi | (qi + KHI)) & ng[b];
                    const unsigned selw = (v[b] >> 1) & 0x03030303u;                     // base codes
                    bad |= (__builtin_amdgcn_perm(LUT, LUT, selw) ^ v[b]) & ff;          // characters other than A, C, G, T
                    inc4 += one;
                    const unsigned tst = 0x03030303u - selw;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned off = __umul24((qi >> (8 * k)) & 0xffu, QF_ROWB) + (((tst >> (8 * k)) & 0xffu) << 7);
                        const unsigned char* cell = lanebase + off;
                        acc[k][0] += *reinterpret_cast<const double*>(cell);
                        acc[k][1] += *reinterpret_cast<const double*>(cell + 128);
                        acc[k][2] += *reinterpret_cast<const double*>(cell + 256);
                        acc[k][3] += *reinterpret_cast<const double*>(cell + 384);
                    }
                }
            }

            // ---- per-column result (accumulators are in code order A, C, T, G) ----
            int nkept = 0;
            int below_kept = 0;
            bool keepk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int inck = static_cast<int>((inc4 >> (8 * k)) & 0xffu);
                keepk[k] = (k < remain) && !(inck < thresh);
                const unsigned long long m = __ballot(keepk[k]);
                below_kept += __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0));
                nkept += __popcll(m);
            }
            emit_columns<true>(A, acc, keepk, obase, outpos + below_kept, g);
            outpos += nkept;
        }
        // every quality string consumed exactly, nothing unusual seen: the group is done
        const bool dirty = __ballot(bad != 0u || (lane < nrows && vpos != qlen)) != 0ull;
        if (lane == 0) {
            A.gflag[g] = dirty ? 1 : 0;
            if (!dirty) A.cons_len[g] = outpos;
        }
    }
}

// ---------------------------------------------------------------------------
// k_consensus_code: the quality vote on rows the MSA stage wrote as 16-bit vote codes (fused multiReadAlign +
// consensusReadSeq).  A code is the index of the cell's (quality, base) entry in the LDS table -- the row writers
// know the read position of every cell, so the quality lookup, the gap / N / alphabet handling and the clamping
// are theirs -- with bit 15 set for a gap.  What is left per cell: one address (code * 128 + the lane's slot), four
// 8-byte LDS reads at immediate offsets, four additions in row order; per row and lane one 8-byte load of four
// codes, independent of everything else, so the next batch of rows is always in flight.  Same sums in the same
// order as the other kernels.
typedef unsigned long long __attribute__((aligned(1))) cons_u64_unaligned;

// The rows of one 256-column step: per row and lane one 8-byte load of four codes, requested one batch of rows
// ahead; per cell one address, four 8-byte LDS reads, four additions.  Loads are unconditional -- rows past the last
// one re-read it, lanes past the row end read its start, both masked afterwards -- so that the compiler can count them
// and wait only for the batch it is about to use.  MASK: the step contains the row end (cells beyond it become gaps).
template <bool MASK>
__device__ __forceinline__ void qc_rows(const uint16_t* rows, long long W, int nrows, int col, int remain, const unsigned char* lanebase,
                                        unsigned long long GAP4, double (&acc)[4][4], unsigned& gaps01, unsigned& gaps23) {
    const unsigned long long keep = !MASK || remain >= 4 ? ~0ull : (remain <= 0 ? 0ull : ((1ull << (16 * remain)) - 1ull));
    const int lcol = (!MASK || remain > 0) ? col : 0;
    unsigned long long wn[QC_RB];
#pragma unroll
    for (int b = 0; b < QC_RB; ++b) wn[b] = *reinterpret_cast<const cons_u64_unaligned*>(rows + static_cast<long long>(min(b, nrows - 1)) * W + lcol);
    for (int r0 = 0; r0 < nrows; r0 += QC_RB) {
        unsigned long long w[QC_RB];
#pragma unroll
        for (int b = 0; b < QC_RB; ++b) w[b] = MASK ? ((wn[b] & keep) | (GAP4 & ~keep)) : wn[b];
#pragma unroll
        for (int b = 0; b < QC_RB; ++b)                 // the next batch (nothing depends on the data)
            wn[b] = *reinterpret_cast<const cons_u64_unaligned*>(rows + static_cast<long long>(min(r0 + QC_RB + b, nrows - 1)) * W + lcol);
#pragma unroll
        for (int b = 0; b < QC_RB; ++b) {
            if (r0 + b >= nrows) break;
            const unsigned lo = static_cast<unsigned>(w[b]), hi = static_cast<unsigned>(w[b] >> 32);
            gaps01 += (lo >> 15) & 0x00010001u;
            gaps23 += (hi >> 15) & 0x00010001u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned h = ((k < 2 ? lo : hi) >> (16 * (k & 1))) & 0x7fffu;
                // four single 8-byte reads (2 LDS cycles each); merged into two ds_read2_b64 they take 8 cycles each
                // (MI355X_MICROARCH.md, LDS table) -- volatile keeps the compiler from pairing them
                typedef const volatile double __attribute__((address_space(3))) lds_cvd;
                lds_cvd* cell = reinterpret_cast<lds_cvd*>(reinterpret_cast<uintptr_t>(lanebase + (h << 7)) & 0xffffffffu);
                const double t0 = cell[0], t1 = cell[16], t2 = cell[32], t3 = cell[48];
                acc[k][0] += t0; acc[k][1] += t1; acc[k][2] += t2; acc[k][3] += t3;
            }
        }
    }
}

__global__ void __launch_bounds__(QF_THREADS) k_consensus_code(const ConsArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    {
        const uint4* src = reinterpret_cast<const uint4*>(A.strip8);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        const int n16 = (A.navail + 1) * (QC_ROWB / 16);
        for (int x = threadIdx.x; x < n16; x += QF_THREADS) dst[x] = src[x];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char* const lanebase = smem + (lane & 15) * 8;
    const unsigned gap1 = CODE_GAPBIT | code_zero_index(A.navail);
    const unsigned long long GAP4 = gap1 * 0x0001000100010001ull;

    for (long long g = static_cast<long long>(blockIdx.x) * (QF_THREADS / 64) + wave; g < A.ngroups;
         g += static_cast<long long>(gridDim.x) * (QF_THREADS / 64)) {
        const long long row0 = A.grp_rows[g];
        const int nrows = static_cast<int>(A.grp_rows[g + 1] - row0);
        if (nrows == 0) {
            if (lane == 0) A.cons_len[g] = 0;
            continue;
        }
        const long long cbase = A.aln_off[row0];
        const long long W = A.aln_off[row0 + 1] - cbase;
        const double thresh = static_cast<double>(nrows) * A.mincov;
        const long long obase = A.out_off[g];
        int outpos = 0;
        const uint16_t* const rows = A.codes + cbase;

        for (long long c0 = 0; c0 < W; c0 += 256) {
            const int col = static_cast<int>(c0) + 4 * lane;
            const int remain = static_cast<int>(W) - col;          // cells of the row at and after `col`
            double acc[4][4];
            unsigned gaps01 = 0, gaps23 = 0;                        // packed 16-bit gap counts of the lane's four columns
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
            // the rows of this step: a variant without the row-end mask for the steps that lie wholly inside the row
            if (c0 + 256 <= W) qc_rows<false>(rows, W, nrows, col, remain, lanebase, GAP4, acc, gaps01, gaps23);
            else qc_rows<true>(rows, W, nrows, col, remain, lanebase, GAP4, acc, gaps01, gaps23);

            // ---- per-column result (accumulators are in code order A, C, T, G) ----
            int nkept = 0;
            int below_kept = 0;
            bool keepk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int inck = nrows - static_cast<int>(((k < 2 ? gaps01 : gaps23) >> (16 * (k & 1))) & 0xffffu);
                keepk[k] = (k < remain) && !(inck < thresh);
                const unsigned long long m = __ballot(keepk[k]);
                below_kept += __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0));
                nkept += __popcll(m);
            }
            emit_columns<false>(A, acc, keepk, obase, outpos + below_kept, g);
            outpos += nkept;
        }
        if (lane == 0) A.cons_len[g] = outpos;
    }
}

// kept columns of every alignment -> contiguous output (one block per alignment)
__global__ void k_consensus_compact(const uint8_t* cons, const uint8_t* phred, const double* lerr, const int64_t* out_off,
                                    const int32_t* len, const long long* dst_off, long long ngroups, uint8_t* dcons,
                                    uint8_t* dphred, double* dlerr) {
    const long long g = blockIdx.x;
    if (g >= ngroups) return;
    const long long src = out_off[g], dst = dst_off[g];
    for (int p = threadIdx.x; p < len[g]; p += blockDim.x) {
        dcons[dst + p] = cons[src + p];
        dphred[dst + p] = phred[src + p];
        if (lerr) dlerr[dst + p] = lerr[src + p];
    }
}

// ---------------------------------------------------------------------------
// One launch of the plan: the LDS attribute, the geometry and the launch all go by the one kernel name.
static int launch(void (*kernel)(const ConsArgs), const ConsLaunch& l, const ConsArgs& a, hipStream_t s) {
    if (l.raise_lds)   // dynamic LDS beyond the default 64 KB
        SL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(l.lds)));
    hipLaunchKernelGGL(kernel, dim3(l.grid), dim3(l.block), l.lds, s, a);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_vote(const ConsPlan& plan, const ConsArgs& a, hipStream_t s) {
    switch (plan.route) {
        case CONS_BASIC: return launch(k_consensus<false>, plan.vote, a, s);
        case CONS_GENERIC: return launch(k_consensus<true>, plan.vote, a, s);
        case CONS_Q4: return launch(k_consensus_q4, plan.vote, a, s);
        case CONS_QF_Q4: {
            // clean groups on the fast kernel (one 1024-thread workgroup per CU around a ~85 KB strip table in LDS);
            // whatever it flags is redone by the generic kernel
            SL_TRY(launch(k_consensus_qf, plan.qf, a, s));
            ConsArgs flagged = a;
            flagged.only_flagged = 1;
            return launch(k_consensus_q4, plan.vote, flagged, s);
        }
        case CONS_CODE: return launch(k_consensus_code, plan.vote, a, s);   // rows written as vote codes by the MSA stage: nothing to decode
    }
    return fail("sarlacc_amd: unknown consensus route %d", static_cast<int>(plan.route));
}

int launch_compact(const ConsArgs& a, const long long* d_dst, uint8_t* d_cons, uint8_t* d_phred, double* d_lerr, hipStream_t s) {
    hipLaunchKernelGGL(k_consensus_compact, dim3(static_cast<unsigned>(a.ngroups)), dim3(256), 0, s, a.cons, a.phred, a.lerr, a.out_off,
                       a.cons_len, d_dst, a.ngroups, d_cons, d_phred, d_lerr);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
