// sam.hip -- SAM alignment records -> ranges, on gfx950 (sam2ranges, /root/reference/R/sam2ranges.R:8-95).
//
// The reference reads the body with read.delim and runs regular expressions over every CIGAR on the host
// (:49-53, :65-74, .get_clip_length :80-95).  Here the body text (everything after the header, which the caller
// reads) is copied to HBM once and parsed there:
//
//   (the line index: k_fq_count, scan, k_fq_lines of text_lines.hip, shared with the FASTQ parser)
//   k_sam_fields   one wavefront per line: the first six tabs by ballots over 64-byte windows, FLAG / MAPQ / POS,
//                  RNAME looked up in a hash table of the @SQ names + '*' + the `restricted` names, the keep
//                  decision, and on kept lines the CIGAR: every lane that holds an op letter reads its digits
//                  backwards, a wave reduction sums the reference-consuming lengths, the first two and last two ops
//                  give the clips.  SEQ, QUAL and the tags are never read.
//   (rocPRIM exclusive scans of the keep flags and of the kept QNAME lengths)
//   k_sam_scatter  kept records -> int32 columns, strand bytes and the name bytes, in file order
//
// A malformed line is reported as k_fq_records does it: atomicMin on (line << 4 | code), read by the host after the
// launch.  No device assert or trap: a bad file is an error return, never a GPU fault.
// Streaming byte work, HBM-bound: 2 reads of the text by the line passes + the fields up to the end of the CIGAR.
// The host side -- the entry points, the name table, the keep / scan back end that bam.hip's records share, the
// messages of the codes (readers.hpp) -- is in readers_host.cpp; the two functions at the end only enqueue.
#include "devprim.hpp"
#include "readers.hpp"

#include <algorithm>
#include <climits>

namespace sarlacc {

// optionally signed decimal integer of at most 2^31 - 1 in magnitude (R's NA_integer_ is -2^31)
__device__ bool parse_i32(const uint8_t* s, long long n, int* out) {
    long long i = 0;
    bool neg = false;
    if (n > 0 && (s[0] == '+' || s[0] == '-')) {
        neg = s[0] == '-';
        i = 1;
    }
    if (i >= n) return false;
    long long v = 0;
    for (; i < n; ++i) {
        const unsigned d = static_cast<unsigned>(s[i]) - '0';
        if (d > 9) return false;
        v = std::min<long long>(v * 10 + d, 1ll << 31);
    }
    if (v > INT_MAX) return false;
    *out = static_cast<int>(neg ? -v : v);
    return true;
}

__device__ __forceinline__ bool is_cigar_op(int c) {
    return c == 'M' || c == 'I' || c == 'D' || c == 'N' || c == 'S' || c == 'H' || c == 'P' || c == '=' || c == 'X';
}
__device__ __forceinline__ bool consumes_ref(int c) { return c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X'; }

// seqinfo code of a name (-1: a `restricted` name that is not in the header, -2: not in the table); *listed: in `restricted`
__device__ int lookup_name(const SamName* table, unsigned long long tmask, const uint8_t* names, const uint8_t* rn, long long rl,
                           int* listed) {
    const unsigned long long h = fnv1a64(rn, rl);
    unsigned long long slot = h & tmask;
    for (unsigned long long probe = 0; probe <= tmask; ++probe, slot = (slot + 1) & tmask) {
        const SamName E = table[slot];
        if (E.len < 0) break;
        if (E.hash == h && E.len == rl) {
            bool eq = true;
            for (long long i = 0; i < rl && eq; ++i) eq = names[E.off + i] == rn[i];
            if (eq) {
                *listed = E.restricted;
                return E.code;
            }
        }
    }
    *listed = 0;
    return -2;
}

constexpr int SAM_THREADS = 256;   // four wavefronts, one line each at a time

__global__ void __launch_bounds__(SAM_THREADS) k_sam_fields(const uint8_t* text, const long long* line_start, long long nlines,
                                                            const SamName* table, unsigned long long tmask, const uint8_t* names,
                                                            int use_restricted, int use_minq, long long minq, SamRec* rec,
                                                            int* keep, long long* name_len, unsigned long long* first_bad) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = static_cast<long long>(gridDim.x) * (SAM_THREADS / 64);
    for (long long k = static_cast<long long>(blockIdx.x) * (SAM_THREADS / 64) + (threadIdx.x >> 6); k < nlines; k += nwaves) {
        const long long b = line_start[k];
        long long e = line_start[k + 1] - 1;                // the newline (or the end of the text)
        if (e > b && text[e - 1] == '\r') --e;              // CRLF files
        int kept = 0, bad = 0;
        long long nlen = 0;
        if (e > b) {                                        // blank lines are skipped
            // the first five tabs: QNAME | FLAG | RNAME | POS | MAPQ | CIGAR ...
            long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
            int ntab = 0;
            for (long long w = b; w < e && ntab < 5; w += 64) {
                const long long p = w + lane;
                unsigned long long m = __ballot(p < e && text[p] == '\t');
                while (m && ntab < 5) {
                    const long long t = w + __builtin_ctzll(m);
                    m &= m - 1;
                    if (ntab == 0) t0 = t; else if (ntab == 1) t1 = t; else if (ntab == 2) t2 = t; else if (ntab == 3) t3 = t; else t4 = t;
                    ++ntab;
                }
            }
            if (ntab < 5) {
                bad = SAM_FIELDS;
            } else {
                // lanes 0-2 parse FLAG, MAPQ and POS; RNAME is looked up by every lane (same addresses: broadcast loads)
                int v = 0, ok = 0;
                if (lane == 0) ok = parse_i32(text + t0 + 1, t1 - t0 - 1, &v);
                else if (lane == 1) ok = parse_i32(text + t3 + 1, t4 - t3 - 1, &v);
                else if (lane == 2) ok = parse_i32(text + t2 + 1, t3 - t2 - 1, &v);
                int listed = 0;
                const int ref = lookup_name(table, tmask, names, text + t1 + 1, t2 - t1 - 1, &listed);
                const int flag = __shfl(v, 0), mapq = __shfl(v, 1), pos = __shfl(v, 2);
                const int flag_ok = __shfl(ok, 0), mapq_ok = __shfl(ok, 1), pos_ok = __shfl(ok, 2);
                if (!flag_ok) bad = SAM_FLAG;
                else if (!mapq_ok) bad = SAM_MAPQ;
                else {
                    kept = !(flag & 4) && (!use_minq || mapq >= minq) && (!use_restricted || (ref != -2 && listed));
                    if (kept && !pos_ok) bad = SAM_POS;
                    else if (kept && ref < 0) bad = SAM_RNAME;
                }
                if (kept && !bad) {
                    // CIGAR from t4 + 1 to the next tab or the end of the line
                    const long long c0 = t4 + 1;
                    long long width = 0;           // per lane, reduced below
                    long long nops = 0, nonclip = 0;
                    int f0t = 0, f1t = 0, l0t = 0, l1t = 0;      // first two / last two op letters (0: none)
                    long long f0l = 0, f1l = 0, l0l = 0, l1l = 0;
                    int carry = 0;                 // last byte of the previous window (0 before the first)
                    long long ce = c0;
                    bool too_long = false;
                    if (e - c0 >= 1 && text[c0] == '*' && (e - c0 == 1 || text[c0 + 1] == '\t')) bad = SAM_CIGAR_STAR;
                    for (long long w = c0; w < e && !bad; w += 64) {
                        const long long p = w + lane;
                        const int c = p < e ? text[p] : 0;
                        const unsigned long long tabs = __ballot(c == '\t');
                        const long long wend = tabs ? w + __builtin_ctzll(tabs) : std::min<long long>(w + 64, e);
                        const bool mine = p < wend;
                        int prev = __shfl_up(c, 1);
                        if (lane == 0) prev = carry;
                        const bool dig = static_cast<unsigned>(c - '0') < 10u;
                        const bool op = mine && is_cigar_op(c);
                        const bool prev_dig = static_cast<unsigned>(prev - '0') < 10u;
                        if (__ballot(mine && !(dig || op) ) || __ballot(op && !prev_dig)) {
                            bad = SAM_CIGAR_SYNTAX;
                            break;
                        }
                        long long len = 0;
                        bool over = false;
                        if (op) {   // digits backwards from p - 1; beyond ten of them only zeros fit in 2^31 - 1
                            long long scale = 1;
                            int i = 0;
                            for (long long q = p - 1; q >= c0; --q, ++i) {
                                const unsigned d = static_cast<unsigned>(text[q]) - '0';
                                if (d > 9) break;
                                if (i < 10) { len += d * scale; scale *= 10; }
                                else if (d) over = true;
                            }
                            over = over || len > INT_MAX;
                            if (consumes_ref(c)) width += len;
                        }
                        too_long = too_long || __ballot(over);   // reported after the syntax of the whole CIGAR
                        const unsigned long long opm = __ballot(op);
                        nonclip += __popcll(__ballot(op && c != 'H' && c != 'S'));
                        if (opm) {
                            if (nops < 2) {
                                const int a = __builtin_ctzll(opm);
                                const unsigned long long rest = opm & (opm - 1);
                                const int a2 = rest ? __builtin_ctzll(rest) : a;
                                const int ta = __shfl(c, a), ta2 = __shfl(c, a2);
                                const long long la = __shfl(len, a), la2 = __shfl(len, a2);
                                if (nops == 0) {
                                    f0t = ta; f0l = la;
                                    if (rest) { f1t = ta2; f1l = la2; }
                                } else {
                                    f1t = ta; f1l = la;
                                }
                            }
                            const int z = 63 - __builtin_clzll(opm);
                            const unsigned long long below = opm & ~(1ull << z);
                            const int z2 = below ? 63 - __builtin_clzll(below) : z;
                            const int tz = __shfl(c, z), tz2 = __shfl(c, z2);
                            const long long lz = __shfl(len, z), lz2 = __shfl(len, z2);
                            if (below) { l1t = tz2; l1l = lz2; }
                            else { l1t = l0t; l1l = l0l; }
                            l0t = tz; l0l = lz;
                            nops += __popcll(opm);
                        }
                        carry = __shfl(c, 63);
                        ce = wend;
                        if (tabs) break;
                    }
                    if (!bad) {
                        // nonempty and ending in an op letter (every op already follows a digit)
                        if (ce <= c0 || !is_cigar_op(text[ce - 1])) bad = SAM_CIGAR_SYNTAX;
                        else if (too_long) bad = SAM_CIGAR_RANGE;
                        else if (nonclip == 0) bad = SAM_CIGAR_CLIPS;
                    }
                    for (int o = 32; o > 0; o >>= 1) width += __shfl_xor(width, o);
                    if (!bad) {
                        // .get_clip_length: a leading (trailing) H, then an S once that H is removed
                        long long lc = 0, rc = 0;
                        if (f0t == 'H') lc = f0l + (f1t == 'S' ? f1l : 0);
                        else if (f0t == 'S') lc = f0l;
                        if (l0t == 'H') rc = l0l + (l1t == 'S' ? l1l : 0);
                        else if (l0t == 'S') rc = l0l;
                        const long long end = static_cast<long long>(pos) + width - 1;
                        if (width > INT_MAX || lc > INT_MAX || rc > INT_MAX) bad = SAM_CIGAR_RANGE;
                        else if (end > INT_MAX || end < -INT_MAX) bad = SAM_END;
                        else if (lane == 0) {
                            SamRec R;
                            R.name_pos = b;
                            R.ref = ref;
                            R.start = pos;
                            R.width = static_cast<int>(width);
                            R.lclip = static_cast<int>(lc);
                            R.rclip = static_cast<int>(rc);
                            R.strand = (flag & 16) ? 1 : 0;
                            rec[k] = R;
                        }
                    }
                    nlen = t0 - b;
                }
            }
        }
        if (bad) kept = 0;
        if (lane == 0) {
            keep[k] = kept;
            name_len[k] = kept ? nlen : 0;
            if (bad) atomicMin(first_bad, (static_cast<unsigned long long>(k) << 4) | static_cast<unsigned>(bad));
        }
    }
}

__global__ void __launch_bounds__(SAM_THREADS) k_sam_scatter(const uint8_t* text, const SamRec* rec, const int* keep,
                                                             const int64_t* koff, const int64_t* noff, long long nlines,
                                                             int32_t* ref, int32_t* start, int32_t* width, uint8_t* strand,
                                                             int32_t* lclip, int32_t* rclip, uint8_t* names, int64_t* name_off) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = static_cast<long long>(gridDim.x) * (SAM_THREADS / 64);
    for (long long k = static_cast<long long>(blockIdx.x) * (SAM_THREADS / 64) + (threadIdx.x >> 6); k < nlines; k += nwaves) {
        if (!keep[k]) continue;
        const long long j = koff[k], no = noff[k], len = noff[k + 1] - no;
        const SamRec R = rec[k];
        if (lane == 0) {
            ref[j] = R.ref; start[j] = R.start; width[j] = R.width;
            strand[j] = R.strand ? '-' : '+';
            lclip[j] = R.lclip; rclip[j] = R.rclip;
            name_off[j] = no;
        }
        for (long long i = lane; i < len; i += 64) names[no + i] = text[R.name_pos + i];
    }
}

// one wavefront per line, up to 256 workgroups per CU
static unsigned sam_grid(long long nlines) {
    return static_cast<unsigned>(std::min<long long>(nblk(nlines, SAM_THREADS / 64), static_cast<long long>(ctx().num_cu) * 256));
}

int sam_fields(const uint8_t* text, const long long* line_start, long long nlines, const SamName* table, unsigned long long tmask,
               const uint8_t* names, int use_restricted, int use_minq, long long minq, SamRec* rec, int* keep,
               long long* name_len, unsigned long long* first_bad, hipStream_t s) {
    hipLaunchKernelGGL(k_sam_fields, dim3(sam_grid(nlines)), dim3(SAM_THREADS), 0, s, text, line_start, nlines, table, tmask, names,
                       use_restricted, use_minq, minq, rec, keep, name_len, first_bad);
    SL_HIP(hipGetLastError());
    return 0;
}

int sam_scatter(const uint8_t* text, const SamRec* rec, const int* keep, const int64_t* koff, const int64_t* noff, long long nlines,
                int32_t* ref, int32_t* start, int32_t* width, uint8_t* strand, int32_t* lclip, int32_t* rclip, uint8_t* names,
                int64_t* name_off, hipStream_t s) {
    hipLaunchKernelGGL(k_sam_scatter, dim3(sam_grid(nlines)), dim3(SAM_THREADS), 0, s, text, rec, keep, koff, noff, nlines, ref,
                       start, width, strand, lclip, rclip, names, name_off);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
