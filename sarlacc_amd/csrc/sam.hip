// sam.hip -- SAM alignment records -> ranges, on gfx950 (sam2ranges, /root/reference/R/sam2ranges.R:8-95).
//
// The reference reads the body with read.delim and runs regular expressions over every CIGAR on the host
// (:49-53, :65-74, .get_clip_length :80-95).  Here the body text (everything after the header, which the caller
// reads) is copied to HBM once and parsed there:
//
//   k_fq_count / k_fq_lines   line index (text_lines.hpp, shared with the FASTQ parser)
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
#include "common.hpp"
#include "devprim.hpp"
#include "sam_rec.hpp"
#include "text_lines.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

namespace sarlacc {

// status codes of a line, in the order the checks run (one code per line; the first bad line wins)
enum {
    SAM_FIELDS = 1,        // non-blank line with fewer than 6 tab-separated fields
    SAM_FLAG = 2,          // FLAG not an optionally signed decimal int32
    SAM_MAPQ = 3,          // MAPQ likewise
    SAM_POS = 4,           // kept line: POS likewise
    SAM_RNAME = 5,         // kept line: RNAME neither an @SQ name nor '*'
    SAM_CIGAR_STAR = 6,    // kept line: CIGAR '*'
    SAM_CIGAR_SYNTAX = 7,  // kept line: CIGAR not ([0-9]+[MIDNSHP=X])+
    SAM_CIGAR_RANGE = 8,   // kept line: an op length, the width or a clip above 2^31 - 1
    SAM_CIGAR_CLIPS = 9,   // kept line: only H / S ops (the reference's right clip is NA)
    SAM_END = 10,          // kept line: start + width - 1 outside the int32 range
};

// one slot of the open-addressing table of reference names (len < 0: empty)
struct SamName {
    unsigned long long hash;
    long long off;      // into the name bytes
    int len;
    int code;           // seqinfo index, -1 for a `restricted` name that is not in the header
    int restricted;     // listed in `restricted`
    int pad;
};

__host__ __device__ __forceinline__ unsigned long long fnv1a64(const uint8_t* s, long long n) {
    unsigned long long h = 14695981039346656037ull;
    for (long long i = 0; i < n; ++i) {
        h ^= s[i];
        h *= 1099511628211ull;
    }
    return h;
}

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

thread_local SamIndex g_sam;   // (sam_rec.hpp; sarlacc_dev_bam_index of bam.hip fills it too)

}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_dev_sam_index(const uint8_t* d_text, int64_t nbytes, int64_t first_line, const char* ref_names,
                          const int64_t* ref_off, int64_t n_ref, const uint8_t* restricted_mask, const char* extra_names,
                          const int64_t* extra_off, int64_t n_extra, int use_minq, int64_t minq, int64_t* n_lines,
                          int64_t* n_kept, int64_t* kept_name_bytes, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0 || n_ref < 0 || n_extra < 0) return fail("sarlacc_amd: negative SAM size");
    if (n_ref >= INT_MAX) return fail("sarlacc_amd: too many reference names");
    hipStream_t s = static_cast<hipStream_t>(stream);
    g_sam = SamIndex{};
    *n_lines = 0; *n_kept = 0; *kept_name_bytes = 0;

    // the name table: seqinfo names (code = index), then the `restricted` names not among them (code -1)
    const int64_t nent = n_ref + n_extra;
    uint64_t tsize = 16;
    while (tsize < 2 * static_cast<uint64_t>(nent) + 2) tsize <<= 1;
    std::vector<SamName> table(tsize, SamName{0, 0, -1, 0, 0, 0});
    std::vector<uint8_t> bytes;
    const uint64_t tmask = tsize - 1;
    for (int64_t i = 0; i < nent; ++i) {
        const bool is_ref = i < n_ref;
        const int64_t j = is_ref ? i : i - n_ref;
        const int64_t* off = is_ref ? ref_off : extra_off;
        const uint8_t* src = reinterpret_cast<const uint8_t*>((is_ref ? ref_names : extra_names) + off[j]);
        const int64_t len = off[j + 1] - off[j];
        if (len < 0 || len >= INT_MAX) return fail("sarlacc_amd: bad reference name offsets");
        const unsigned long long h = fnv1a64(src, len);
        uint64_t slot = h & tmask;
        bool dup = false;
        for (; table[slot].len >= 0; slot = (slot + 1) & tmask) {
            const SamName& E = table[slot];
            if (E.hash == h && E.len == len && std::equal(src, src + len, bytes.data() + E.off)) { dup = true; break; }
        }
        if (dup) {
            if (is_ref) return fail("duplicate @SQ name '%.*s'", static_cast<int>(std::min<int64_t>(len, 200)), src);
            continue;   // a restricted name listed twice, or one that is also a seqinfo name
        }
        table[slot] = SamName{h, static_cast<long long>(bytes.size()), static_cast<int>(len), is_ref ? static_cast<int>(i) : -1,
                              is_ref ? (restricted_mask ? restricted_mask[i] != 0 : 0) : 1, 0};
        bytes.insert(bytes.end(), src, src + len);
    }
    if (nbytes == 0) {
        g_sam.text = d_text;   // no lines: an empty result
        return 0;
    }

    // line index, as the FASTQ parser builds it
    const long long ntiles = (nbytes + FQ_TILE - 1) / FQ_TILE;
    long long* d_count; long long* d_base;
    SL_TRY(scratch("fq.count", static_cast<size_t>(ntiles) + 1, &d_count));
    SL_TRY(scratch("fq.base", static_cast<size_t>(ntiles) + 1, &d_base));
    SL_HIP(hipMemsetAsync(d_count + ntiles, 0, sizeof(long long), s));
    hipLaunchKernelGGL(k_fq_count, dim3(static_cast<unsigned>(ntiles)), dim3(FQ_THREADS), 0, s, d_text, static_cast<long long>(nbytes), d_count);
    SL_HIP(hipGetLastError());
    SL_TRY(exclusive_scan("fq.scan", d_count, reinterpret_cast<int64_t*>(d_base), static_cast<size_t>(ntiles) + 1, s));
    long long newlines = 0;
    uint8_t last = 0;
    SL_HIP(hipMemcpyAsync(&newlines, d_base + ntiles, sizeof newlines, hipMemcpyDeviceToHost, s));
    SL_HIP(hipMemcpyAsync(&last, d_text + nbytes - 1, 1, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    // one more line than newlines; after a final newline that line is empty, i.e. blank
    const long long nlines = newlines + 1;

    long long* d_lines; SamName* d_table; uint8_t* d_names;
    SL_TRY(scratch("sam.lines", static_cast<size_t>(nlines) + 1, &d_lines));
    const long long zero = 0, end = nbytes + 1;
    SL_HIP(hipMemcpyAsync(d_lines, &zero, sizeof zero, hipMemcpyHostToDevice, s));
    SL_HIP(hipMemcpyAsync(d_lines + nlines, &end, sizeof end, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fq_lines, dim3(static_cast<unsigned>(ntiles)), dim3(FQ_THREADS), 0, s, d_text, static_cast<long long>(nbytes), d_base, d_lines);
    SL_HIP(hipGetLastError());
    SL_TRY(upload("sam.table", table.data(), table.size(), &d_table, s));
    SL_TRY(upload("sam.names", bytes.data(), bytes.size(), &d_names, s));

    SamRec* d_rec; int* d_keep; long long* d_nlen; int64_t* d_koff; int64_t* d_noff; unsigned long long* d_bad;
    SL_TRY(scratch("sam.rec", static_cast<size_t>(nlines), &d_rec));
    SL_TRY(scratch("sam.keep", static_cast<size_t>(nlines) + 1, &d_keep));
    SL_TRY(scratch("sam.nlen", static_cast<size_t>(nlines) + 1, &d_nlen));
    SL_TRY(scratch("sam.koff", static_cast<size_t>(nlines) + 1, &d_koff));
    SL_TRY(scratch("sam.noff", static_cast<size_t>(nlines) + 1, &d_noff));
    SL_TRY(scratch("sam.bad", 1, &d_bad));
    SL_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), s));
    SL_HIP(hipMemsetAsync(d_keep + nlines, 0, sizeof(int), s));
    SL_HIP(hipMemsetAsync(d_nlen + nlines, 0, sizeof(long long), s));
    Context& c = ctx();
    const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(nlines, SAM_THREADS / 64), static_cast<long long>(c.num_cu) * 256));
    hipLaunchKernelGGL(k_sam_fields, dim3(grid), dim3(SAM_THREADS), 0, s, d_text, d_lines, nlines, d_table,
                       static_cast<unsigned long long>(tmask), d_names, restricted_mask ? 1 : 0, use_minq ? 1 : 0,
                       static_cast<long long>(minq), d_rec, d_keep, d_nlen, d_bad);
    SL_HIP(hipGetLastError());
    SL_TRY(exclusive_scan("sam.scan", d_keep, d_koff, static_cast<size_t>(nlines) + 1, s));
    SL_TRY(exclusive_scan("sam.scan", d_nlen, d_noff, static_cast<size_t>(nlines) + 1, s));
    unsigned long long bad = 0;
    int64_t nk = 0, nb = 0;
    SL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SL_HIP(hipMemcpyAsync(&nk, d_koff + nlines, sizeof nk, hipMemcpyDeviceToHost, s));
    SL_HIP(hipMemcpyAsync(&nb, d_noff + nlines, sizeof nb, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) {
        const long long line = first_line + static_cast<long long>(bad >> 4);
        switch (bad & 15u) {
            case SAM_FIELDS: return fail("SAM line %lld: fewer than 6 tab-separated fields", line);
            case SAM_FLAG: return fail("SAM line %lld: FLAG is not a 32-bit integer", line);
            case SAM_MAPQ: return fail("SAM line %lld: MAPQ is not a 32-bit integer", line);
            case SAM_POS: return fail("SAM line %lld: POS is not a 32-bit integer", line);
            case SAM_RNAME: return fail("SAM line %lld: RNAME is neither an @SQ name nor '*'", line);
            case SAM_CIGAR_STAR: return fail("SAM line %lld: CIGAR '*' on a kept record", line);
            case SAM_CIGAR_SYNTAX: return fail("SAM line %lld: CIGAR does not match ([0-9]+[MIDNSHP=X])+", line);
            case SAM_CIGAR_RANGE: return fail("SAM line %lld: CIGAR length above 2^31 - 1", line);
            case SAM_CIGAR_CLIPS: return fail("SAM line %lld: CIGAR has only H and S operations", line);
            default: return fail("SAM line %lld: alignment end outside the 32-bit integer range", line);
        }
    }
    g_sam.text = d_text; g_sam.nlines = nlines; g_sam.nkept = nk; g_sam.name_bytes = nb;
    *n_lines = newlines + (last != '\n' ? 1 : 0);
    *n_kept = nk; *kept_name_bytes = nb;
    return 0;
}

int sarlacc_dev_sam_extract(const uint8_t* d_text, int32_t* d_ref, int32_t* d_start, int32_t* d_width, uint8_t* d_strand,
                            int32_t* d_lclip, int32_t* d_rclip, uint8_t* d_names, int64_t* d_name_off, void* stream) {
    SL_TRY(ensure_device());
    if (!d_text || d_text != g_sam.text) return fail("sarlacc_amd: sarlacc_dev_sam_extract without a matching sarlacc_dev_sam_index");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nlines = g_sam.nlines, nk = g_sam.nkept, nb = g_sam.name_bytes;
    SL_HIP(hipMemcpyAsync(d_name_off + nk, &nb, sizeof nb, hipMemcpyHostToDevice, s));
    if (nk > 0) {
        SamRec* d_rec; int* d_keep; int64_t* d_koff; int64_t* d_noff;
        SL_TRY(scratch("sam.rec", static_cast<size_t>(nlines), &d_rec));
        SL_TRY(scratch("sam.keep", static_cast<size_t>(nlines) + 1, &d_keep));
        SL_TRY(scratch("sam.koff", static_cast<size_t>(nlines) + 1, &d_koff));
        SL_TRY(scratch("sam.noff", static_cast<size_t>(nlines) + 1, &d_noff));
        Context& c = ctx();
        const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(nlines, SAM_THREADS / 64), static_cast<long long>(c.num_cu) * 256));
        c.stage_reset("sam_scatter");
        SL_TRY(c.stage_begin("sam_scatter", s));
        hipLaunchKernelGGL(k_sam_scatter, dim3(grid), dim3(SAM_THREADS), 0, s, d_text, d_rec, d_keep, d_koff, d_noff,
                           static_cast<long long>(nlines), d_ref, d_start, d_width, d_strand, d_lclip, d_rclip, d_names, d_name_off);
        SL_HIP(hipGetLastError());
        SL_TRY(c.stage_end("sam_scatter", s));
    }
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}
}
