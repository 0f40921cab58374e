// bgzf_deflate.hip -- device text -> BGZF (blocked gzip, SAM specification section 4.1; RFC 1951 / RFC 1952) on gfx950:
// a Huffman-only deflate encoder with, where that is smaller, a code table per line.  The writer's side of bgzf.hip.
//
//   sarlacc_bgzf_deflate_bound   host: number of blocks and the capacity the output needs
//   k_bgzf_deflate               one wavefront per BGZF block (one 64-thread workgroup each, assigned statically):
//                                header, deflate payload, CRC-32 and ISIZE into the block's own 64-KB slot
//   (rocPRIM exclusive scan over the block sizes: n + 1 offsets)
//   k_bgzf_pack                  the slots made contiguous, 16 bytes per store
//
// Block k holds the text bytes [k * 65280, min((k + 1) * 65280, n)) (0xff00, htslib's choice: the stored form of a full
// block, 18 + 5 + 65280 + 8 bytes, stays within BSIZE's 65536).  FASTQ text is nearly memoryless, so matching gains
// little (4 % at zlib's level 6 on 2-kb reads) while a code per line gains a lot: a sequence line wants 2 bits per
// base, a quality line about 3.7, and one shared table charges each about a bit more.  Symbols are literals and
// end-of-block only; every table declares one distance code of length 0, which inflate takes as "no distances".
//
// Candidates per BGZF block, compared by their exact bit counts (table headers included), ties to the earlier one:
//   (a) one dynamic-Huffman deflate block for the whole BGZF block
//   (b) one dynamic-Huffman deflate block per PIECE.  A piece ends behind a newline (byte 10) or at the block's end;
//       a newline that would close a piece of fewer than 64 bytes does not close it, so "+\n" goes with the quality
//       line behind it and a short name line with its sequence.  A line that began in the previous block is simply
//       the block's first piece.  Bytes without lines (BAM records, bam_write.hip) come with the caller's own CUTS
//       (sarlacc_dev_bgzf_deflate_cuts): a piece then ends at the first cut that lies at least 64 bytes into it, found
//       by a binary search in the sorted cuts, the same in every lane; newlines play no part.
//   (c) one stored deflate block: the floor for incompressible bytes, and why everything fits in a slot
// (b) needs no state per line: the pieces are encoded one after the other straight into the slot, and the attempt is
// given up before the piece whose bits would bring the running total to the smaller of (a) and (c) -- so 32640 lines
// of "+\n" cost a few pieces, not 32640 tables, nothing written passes the stored size, and no cap on the number of
// lines is needed.  If (b) is given up, the slot is written again from its start with (a) or (c).
//
// A code (build_code): the used symbols are compacted (ballot), ranked by count (every lane counts the symbols below
// its own: m * ceil(m / 64) broadcast reads of LDS), merged by lane 0 with the two-queue method (sorted leaves, internal
// nodes in creation order: Huffman-optimal), the depths cut at the limit (15 bits; 7 for the code-length code) and the
// Kraft sum repaired on the counts per length (one code leaves the longest length, one code one level up takes a
// sibling, until the sum is exactly one: a complete prefix code), lengths handed out by rank, canonical codes by the
// number of lower symbols of the same length.  The table header run-length codes the 258 lengths with the symbols
// 16, 17 and 18, one lane per run.
//
// Emission: 64 bytes a step; the lengths and bit-reversed codes come from a 257-entry LDS table, a wavefront prefix sum
// gives every byte its bit position, the codes are OR-ed (LDS atomics: the result does not depend on their order)
// into a staging window of 160 words whose bit 0 is the slot's byte 16, so that whole words leave for 16-byte aligned
// places: full groups of four words as one 16-byte store, the ends of a flush word by word.  The two BSIZE bytes
// that share the first word are written last.
//
// Bounds: every loop runs over the bytes of a piece, the used symbols (at most 257) or the lengths (258); the staging
// window holds at most 63 full words when a step begins, a step adds at most 64 * 15 bits, a table header at most
// 3 + 14 + 57 + 258 * 7 bits after a full flush.  No spin-wait, no dependence between workgroups, no printf/assert,
// no racing stores: the same text and mode give the same bytes.
//
// Out of scope: LZ77 matching (the measured gain on long reads is the 4 % above: a follow-up of its own),
// .gzi / .csi indexes, compressing on the host.
#include "common.hpp"
#include "crc32.hpp"
#include "out_tiles.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>

namespace sarlacc {
namespace {

constexpr int DF_BLOCK = 0xff00;         // text bytes per BGZF block
constexpr int DF_SLOT = 65536;           // bytes a block is encoded into
constexpr int DF_MIN_PIECE = 64;         // a newline closes a piece only from this many bytes on
constexpr int DF_STAGE = 160;            // words of the staging window
constexpr int DF_FLUSH = 64;             // full words that trigger a flush
constexpr int DF_NLEN = 258;             // lengths a table header codes: 257 literal/length codes and one distance code
constexpr int DF_ORIGIN = 16;            // slot byte of the staging window's bit 0 (the payload starts at byte 18)

__constant__ uint8_t c_df_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DfShared {
    uint32_t cnt[257];         // histogram of the piece: 256 literals and end-of-block
    uint32_t tab[257];         // bit-reversed code << 5 | length
    uint8_t lens[DF_NLEN + 2]; // code lengths by symbol; [257] is the distance code's 0
    uint32_t ccnt[19];         // the code-length code: histogram, table, lengths
    uint32_t ctab[19];
    uint8_t clens[20];
    uint16_t run_start[DF_NLEN + 2];
    // build_code's work space
    uint16_t us[257];          // used symbols, ascending
    uint32_t uc[257];          // their counts
    uint16_t so[257];          // rank by count -> index in us
    uint32_t sc[257];          // counts by rank
    uint32_t iw[256];          // weights of the internal nodes, in creation order
    uint16_t lp[257], ip[256]; // parent (an internal node) of a leaf by rank, of an internal node
    uint8_t idp[256];          // depth of an internal node
    uint8_t ul[260];           // code length by index in us
    uint32_t bl[16], nc[16];   // codes per length, first canonical code of a length
    uint32_t stage[DF_STAGE];
    uint32_t crc_table[256];
};

__device__ __forceinline__ void fence_wave() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_scan(int v, int lane) {   // inclusive
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// Code lengths (at most maxbits) and codes of the symbols with cnt[s] > 0, s < nsym; lens[s] = 0 and tab[s] = 0 for
// the others.  All lanes; returns the number of used symbols.
__device__ int build_code(DfShared& sh, const uint32_t* cnt, int nsym, int maxbits, uint8_t* lens, uint32_t* tab, int lane) {
    int m = 0;
    for (int base = 0; base < nsym; base += 64) {
        const int s = base + lane;
        const uint32_t c = s < nsym ? cnt[s] : 0u;
        const unsigned long long used = __ballot(c > 0);
        if (c > 0) {
            const int p = m + __popcll(used & ((1ull << lane) - 1));
            sh.us[p] = static_cast<uint16_t>(s);
            sh.uc[p] = c;
        }
        if (s < nsym) { lens[s] = 0; tab[s] = 0; }
        m += __popcll(used);
    }
    fence_wave();
    if (m == 0) return 0;
    if (m == 1) {          // (a lone code of one bit; neither caller has fewer than two symbols)
        if (lane == 0) { lens[sh.us[0]] = 1; tab[sh.us[0]] = 1; }
        fence_wave();
        return 1;
    }
    // rank by (count, symbol)
    for (int j = lane; j < m; j += 64) {
        const uint32_t c = sh.uc[j];
        int r = 0;
        for (int i = 0; i < m; ++i) {
            const uint32_t ci = sh.uc[i];
            r += (ci < c || (ci == c && i < j)) ? 1 : 0;
        }
        sh.so[r] = static_cast<uint16_t>(j);
        sh.sc[r] = c;
    }
    if (lane < 16) sh.bl[lane] = 0;
    fence_wave();
    if (lane == 0) {
        // two queues: leaves by rank, internal nodes by creation; a leaf goes first at equal weight
        int li = 0, ii = 0;
        for (int t = 0; t < m - 1; ++t) {
            uint32_t w = 0;
            for (int k = 0; k < 2; ++k) {
                const bool leaf = li < m && (ii >= t || sh.sc[li] <= sh.iw[ii]);
                if (leaf) { w += sh.sc[li]; sh.lp[li] = static_cast<uint16_t>(t); ++li; }
                else { w += sh.iw[ii]; sh.ip[ii] = static_cast<uint16_t>(t); ++ii; }
            }
            sh.iw[t] = w;
        }
        sh.idp[m - 2] = 0;
        for (int k = m - 3; k >= 0; --k) sh.idp[k] = static_cast<uint8_t>(sh.idp[sh.ip[k]] + 1);
    }
    fence_wave();
    for (int j = lane; j < m; j += 64) {
        const int l = min(static_cast<int>(sh.idp[sh.lp[j]]) + 1, maxbits);
        atomicAdd(&sh.bl[l], 1u);
    }
    fence_wave();
    if (lane == 0) {
        // Kraft sum in units of 2^-maxbits; every turn takes one unit off
        uint32_t total = 0;
        for (int l = 1; l <= maxbits; ++l) total += sh.bl[l] << (maxbits - l);
        while (total > (1u << maxbits)) {
            sh.bl[maxbits]--;
            for (int i = maxbits - 1; i > 0; --i)
                if (sh.bl[i]) { sh.bl[i]--; sh.bl[i + 1] += 2; break; }
            --total;
        }
        uint32_t code = 0;
        for (int l = 1; l <= maxbits; ++l) { sh.nc[l] = code; code = (code + sh.bl[l]) << 1; }
    }
    fence_wave();
    // the rarest symbols take the longest codes
    for (int r = lane; r < m; r += 64) {
        int acc = 0, l = maxbits;
        for (; l > 1; --l) {
            acc += static_cast<int>(sh.bl[l]);
            if (r < acc) break;
        }
        sh.ul[sh.so[r]] = static_cast<uint8_t>(l);
    }
    fence_wave();
    for (int j = lane; j < m; j += 64) {
        const int l = sh.ul[j];
        int rk = 0;
        for (int i = 0; i < j; ++i) rk += sh.ul[i] == l ? 1 : 0;
        const uint32_t code = sh.nc[l] + static_cast<uint32_t>(rk);
        const int s = sh.us[j];
        lens[s] = static_cast<uint8_t>(l);
        tab[s] = ((__brev(code) >> (32 - l)) << 5) | static_cast<uint32_t>(l);
    }
    fence_wave();
    return m;
}

// The tokens of a run of n equal lengths v, as zlib cuts them: f(symbol, extra bits' value, their number)
template <class F>
__device__ __forceinline__ void run_tokens(int v, int n, F f) {
    if (v == 0) {
        while (n >= 11) { const int k = min(n, 138); f(18, k - 11, 7); n -= k; }
        if (n >= 3) { f(17, n - 3, 3); n = 0; }
        for (; n > 0; --n) f(0, 0, 0);
    } else {
        f(v, 0, 0);
        --n;
        while (n >= 3) { const int k = min(n, 6); f(16, k - 3, 2); n -= k; }
        for (; n > 0; --n) f(v, 0, 0);
    }
}

// the bit stream of a slot's payload as it is being written
struct DfOut {
    uint32_t* words;   // the slot from byte DF_ORIGIN on
    int wbase;         // word of the stream that stage[0] is
    int pos;           // bits written (from byte DF_ORIGIN)
};

__device__ __forceinline__ void put_bits(DfShared& sh, const DfOut& o, int pos, uint32_t v, int n) {
    if (n == 0) return;
    const int rel = pos - (o.wbase << 5);
    const uint64_t x = static_cast<uint64_t>(v) << (rel & 31);
    atomicOr(&sh.stage[rel >> 5], static_cast<uint32_t>(x));
    if (x >> 32) atomicOr(&sh.stage[(rel >> 5) + 1], static_cast<uint32_t>(x >> 32));
}

// Whole words of the window to the slot (all: the last, partial one too); the partial word moves to stage[0].  All lanes.
__device__ void flush(DfShared& sh, DfOut& o, bool all, int lane) {
    fence_wave();
    const int wend = all ? (o.pos + 31) >> 5 : o.pos >> 5;
    const int nfull = wend - o.wbase;
    if (nfull <= 0) return;
    const uint32_t partial = all ? 0u : sh.stage[nfull];
    for (int g = (o.wbase >> 2) + lane; g < (wend + 3) >> 2; g += 64) {
        const int a = g * 4;
        if (a >= o.wbase && a + 4 <= wend) {
            const uint32_t* p = &sh.stage[a - o.wbase];
            u32x4 v;
            v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
            *reinterpret_cast<u32x4*>(o.words + a) = v;
        } else {
            for (int j = 0; j < 4; ++j)
                if (a + j >= o.wbase && a + j < wend) o.words[a + j] = sh.stage[a + j - o.wbase];
        }
    }
    fence_wave();
    for (int s = lane; s <= nfull && s < DF_STAGE; s += 64) sh.stage[s] = s == 0 ? partial : 0u;
    fence_wave();
    o.wbase = wend;
}

// Histogram, code and table header of the bytes [b, e) of the block.  Returns the exact bits of the deflate block
// (3 + header + payload + end-of-block); leaves tab / lens / ctab / clens / run_start for emit_piece.  *hclen, *nruns out.
__device__ int prepare_piece(DfShared& sh, const uint8_t* text, int b, int e, int* hclen, int* nruns, int lane) {
    for (int s = lane; s < 257; s += 64) sh.cnt[s] = s == 256 ? 1u : 0u;
    if (lane < 19) sh.ccnt[lane] = 0;
    fence_wave();
    for (int i = b + lane; i < e; i += 64) atomicAdd(&sh.cnt[text[i]], 1u);
    fence_wave();
    build_code(sh, sh.cnt, 257, 15, sh.lens, sh.tab, lane);
    if (lane == 0) sh.lens[257] = 0;
    fence_wave();
    int payload = 0;
    for (int s = lane; s < 257; s += 64) payload += static_cast<int>(sh.cnt[s]) * sh.lens[s];
    payload = wave_sum(payload);
    // runs of equal lengths
    int R = 0;
    for (int base = 0; base < DF_NLEN; base += 64) {
        const int i = base + lane;
        const bool start = i < DF_NLEN && (i == 0 || sh.lens[i - 1] != sh.lens[i]);
        const unsigned long long st = __ballot(start);
        if (start) sh.run_start[R + __popcll(st & ((1ull << lane) - 1))] = static_cast<uint16_t>(i);
        R += __popcll(st);
    }
    if (lane == 0) sh.run_start[R] = DF_NLEN;
    fence_wave();
    int extra = 0;
    for (int r = lane; r < R; r += 64) {
        const int s = sh.run_start[r];
        run_tokens(sh.lens[s], sh.run_start[r + 1] - s, [&](int sym, int, int nx) {
            atomicAdd(&sh.ccnt[sym], 1u);
            extra += nx;
        });
    }
    extra = wave_sum(extra);
    fence_wave();
    build_code(sh, sh.ccnt, 19, 7, sh.clens, sh.ctab, lane);
    int last = 3;
    for (int i = 4; i < 19; ++i)
        if (sh.clens[c_df_clen_order[i]]) last = i;
    *hclen = last + 1;
    *nruns = R;
    int hdr = lane < 19 ? static_cast<int>(sh.ccnt[lane]) * sh.clens[lane] : 0;
    hdr = wave_sum(hdr);
    return 3 + 14 + 3 * (last + 1) + hdr + extra + payload;
}

// The deflate block prepare_piece sized, into the stream.  All lanes.
__device__ void emit_piece(DfShared& sh, DfOut& o, const uint8_t* text, int b, int e, bool final, int hclen, int nruns, int lane) {
    flush(sh, o, false, lane);
    // BFINAL, BTYPE 2, HLIT 0 (257 codes), HDIST 0 (1 code), HCLEN
    if (lane == 0) put_bits(sh, o, o.pos, (final ? 1u : 0u) | (2u << 1) | (static_cast<uint32_t>(hclen - 4) << 13), 17);
    if (lane < hclen) put_bits(sh, o, o.pos + 17 + 3 * lane, sh.clens[c_df_clen_order[lane]], 3);
    o.pos += 17 + 3 * hclen;
    for (int base = 0; base < nruns; base += 64) {
        const int r = base + lane;
        int s = 0, n = 0, v = 0, bits = 0;
        if (r < nruns) {
            s = sh.run_start[r];
            n = sh.run_start[r + 1] - s;
            v = sh.lens[s];
            run_tokens(v, n, [&](int sym, int, int nx) { bits += sh.clens[sym] + nx; });
        }
        const int incl = wave_scan(bits, lane);
        int p = o.pos + incl - bits;
        if (r < nruns)
            run_tokens(v, n, [&](int sym, int x, int nx) {
                const uint32_t t = sh.ctab[sym];
                const int l = static_cast<int>(t & 31u);
                put_bits(sh, o, p, (t >> 5) | (static_cast<uint32_t>(x) << l), l + nx);
                p += l + nx;
            });
        o.pos += __shfl(incl, 63);
    }
    // (the bits were counted before and lie below the stored size; the test keeps a miscount inside the slot)
    for (int i0 = b; i0 < e && o.pos < (DF_SLOT - DF_ORIGIN - 256) * 8; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t t = i < e ? sh.tab[text[i]] : 0u;
        const int l = static_cast<int>(t & 31u);
        const int incl = wave_scan(l, lane);
        put_bits(sh, o, o.pos + incl - l, t >> 5, l);
        o.pos += __shfl(incl, 63);
        if ((o.pos >> 5) - o.wbase >= DF_FLUSH) flush(sh, o, false, lane);
    }
    const uint32_t eob = sh.tab[256];
    if (lane == 0) put_bits(sh, o, o.pos, eob >> 5, static_cast<int>(eob & 31u));
    o.pos += static_cast<int>(eob & 31u);
}

__device__ __forceinline__ void reset_stream(DfShared& sh, DfOut& o, int lane) {
    fence_wave();
    for (int s = lane; s < DF_STAGE; s += 64) sh.stage[s] = 0;
    fence_wave();
    o.wbase = 0;
    o.pos = (18 - DF_ORIGIN) * 8;
}

// mode: 0 = smallest of (a), (b), (c); 1 = (a) or (c); 2 = (c).  CUTS: the pieces of (b) end at the caller's cuts
// (cuts[j] - cut_origin is a position in the whole text), not behind newlines.
template <bool CUTS>
__global__ void __launch_bounds__(64) k_bgzf_deflate(const uint8_t* __restrict__ text_all, long long nbytes, long long nblocks,
                                                     int mode, const int64_t* __restrict__ cuts, long long n_cuts,
                                                     long long cut_origin, uint8_t* __restrict__ slots,
                                                     int64_t* __restrict__ size) {
    __shared__ DfShared sh;
    const long long k = blockIdx.x;
    if (k >= nblocks) return;
    const int lane = threadIdx.x;
    const uint8_t* text = text_all + k * DF_BLOCK;
    const int n = static_cast<int>(min(static_cast<long long>(DF_BLOCK), nbytes - k * DF_BLOCK));   // 1 .. 65280
    uint8_t* slot = slots + k * DF_SLOT;

    // CRC-32 of the text: 64 slices, shifted to the end and folded (as k_bgzf_crc)
    for (int i = lane; i < 256; i += 64) sh.crc_table[i] = crc_table_entry(i);
    fence_wave();
    uint32_t crc;
    {
        const int slice = (n + 63) / 64;
        const int b = min(lane * slice, n), e = min(b + slice, n);
        uint32_t c = 0xffffffffu;
        for (int i = b; i < e; ++i) c = sh.crc_table[(c ^ text[i]) & 0xffu] ^ (c >> 8);
        c = e > b ? ~c : 0u;
        c = crc_shift(c, static_cast<uint32_t>(n - e));
        for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o);
        crc = c;
    }

    DfOut out{reinterpret_cast<uint32_t*>(slot + DF_ORIGIN), 0, 0};
    reset_stream(sh, out, lane);
    const int start_pos = out.pos;
    const int c_bits = 8 * (5 + n);
    int hclen = 0, nruns = 0;
    int a_bits = 0x7fffffff;
    if (mode != 2) a_bits = prepare_piece(sh, text, 0, n, &hclen, &nruns, lane);
    const int best = min(a_bits, c_bits);
    int choice = a_bits <= c_bits ? 0 : 2;
    if (mode == 0) {
        bool won = true;
        int b = 0;
        while (b < n) {
            int e = n;
            if constexpr (CUTS) {
                // the piece ends at the first cut at b + DF_MIN_PIECE or later (the same search in every lane)
                const long long want = cut_origin + k * DF_BLOCK + b + DF_MIN_PIECE;
                long long lo = 0, hi = n_cuts;      // cuts[j] < want for j < lo, >= want for j >= hi
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (cuts[mid] < want) lo = mid + 1; else hi = mid;
                }
                if (lo < n_cuts) {
                    const long long at = cuts[lo] - cut_origin - k * DF_BLOCK;
                    if (at < n) e = static_cast<int>(at);
                }
            } else {
                // the piece ends behind the first newline at b + DF_MIN_PIECE - 1 or later
                for (int i0 = b + DF_MIN_PIECE - 1; i0 < n; i0 += 64) {
                    const int i = i0 + lane;
                    const unsigned long long nl = __ballot(i < n && text[i] == 10);
                    if (nl) { e = i0 + __ffsll(static_cast<long long>(nl)); break; }
                }
            }
            const int bits = prepare_piece(sh, text, b, e, &hclen, &nruns, lane);
            if (out.pos - start_pos + bits >= best) { won = false; break; }
            emit_piece(sh, out, text, b, e, e == n, hclen, nruns, lane);
            b = e;
        }
        if (won) choice = 1;
        else reset_stream(sh, out, lane);
    }
    int pay_bytes;
    if (choice == 0) {
        if (mode == 0) prepare_piece(sh, text, 0, n, &hclen, &nruns, lane);   // the pieces used the tables
        emit_piece(sh, out, text, 0, n, true, hclen, nruns, lane);
    }
    if (choice != 2) {
        pay_bytes = (out.pos - start_pos + 7) >> 3;
        flush(sh, out, true, lane);
    } else {
        pay_bytes = 5 + n;
        if (lane < 5) {
            const uint32_t len = static_cast<uint32_t>(n), nlen = ~len & 0xffffu;
            slot[18 + lane] = lane == 0 ? 1 : lane == 1 ? len & 0xff : lane == 2 ? len >> 8 : lane == 3 ? nlen & 0xff : nlen >> 8;
        }
        for (int i = lane; i < n; i += 64) slot[23 + i] = text[i];
    }
    fence_wave();
    // the gzip member around it: header with the BC subfield, CRC-32, ISIZE
    const int total = 18 + pay_bytes + 8;
    if (lane < 18) {
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        slot[lane] = lane < 16 ? head[lane] : static_cast<uint8_t>((total - 1) >> (8 * (lane - 16)));
    } else if (lane < 26) {
        const int j = lane - 18;
        const uint32_t v = j < 4 ? crc : static_cast<uint32_t>(n);
        slot[18 + pay_bytes + j] = static_cast<uint8_t>(v >> (8 * (j & 3)));
    }
    if (lane == 0) size[k] = total;
}

// comp[0 .. off[nblocks]) = the blocks side by side; work divided by 16-byte aligned pieces of the output
__global__ void __launch_bounds__(256) k_bgzf_pack(const uint8_t* __restrict__ slots, const int64_t* __restrict__ off,
                                                   long long nblocks, uint8_t* __restrict__ comp) {
    const long long total = off[nblocks];
    const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(comp) & 15);
    const long long npieces = (total + mis + 15) / 16;
    const long long nthreads = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long p = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; p < npieces; p += nthreads) {
        const long long p0 = p * 16 - mis;
        const long long v0 = p0 > 0 ? p0 : 0, v1 = p0 + 16 < total ? p0 + 16 : total;
        if (v0 >= v1) continue;
        long long k = last_not_above(off, 0, nblocks, v0);
        if (v1 - v0 == 16 && v1 <= off[k + 1]) {
            *reinterpret_cast<u32x4*>(comp + v0) = *reinterpret_cast<const u32x4_unaligned*>(slots + k * DF_SLOT + (v0 - off[k]));
            continue;
        }
        for (long long q = v0; q < v1; ++q) {
            while (q >= off[k + 1]) ++k;     // every block has at least 27 bytes
            comp[q] = slots[k * DF_SLOT + (q - off[k])];
        }
    }
}

int bgzf_deflate_bound(int64_t nbytes, int64_t* n_blocks, int64_t* comp_capacity) {
    if (nbytes < 0) return fail("sarlacc_amd: negative text size");
    const int64_t n = (nbytes + DF_BLOCK - 1) / DF_BLOCK;
    if (n_blocks) *n_blocks = n;
    if (comp_capacity) *comp_capacity = n * DF_SLOT;
    return 0;
}

// both entry points; use_cuts: the pieces end at d_cuts (which may be NULL for n_cuts == 0), not behind newlines
int bgzf_deflate(const uint8_t* d_text, int64_t nbytes, bool use_cuts, const int64_t* d_cuts, int64_t n_cuts, int64_t cut_origin,
                 int mode, uint8_t* d_comp, int64_t comp_capacity, int64_t* d_comp_off, int64_t* comp_bytes, hipStream_t s) {
    int64_t n_blocks = 0, need = 0;
    SL_TRY(bgzf_deflate_bound(nbytes, &n_blocks, &need));
    if (mode < 0 || mode > 2) return fail("sarlacc_amd: unknown BGZF deflate mode %d", mode);
    if (n_cuts < 0 || (n_cuts > 0 && !d_cuts)) return fail("sarlacc_amd: bad BGZF deflate cuts");
    if (comp_capacity < need)
        return fail("sarlacc_amd: BGZF output capacity %lld is below the bound %lld", static_cast<long long>(comp_capacity),
                    static_cast<long long>(need));
    if (!comp_bytes) return fail("sarlacc_amd: bad BGZF deflate request");
    *comp_bytes = 0;
    SL_TRY(ensure_device());
    if (nbytes == 0) {
        if (d_comp_off) {
            SL_HIP(hipMemsetAsync(d_comp_off, 0, sizeof(int64_t), s));
            SL_HIP(hipStreamSynchronize(s));
        }
        return 0;
    }
    if (n_blocks > 0x7fffffffLL) return fail("sarlacc_amd: more than 2^31 - 1 BGZF blocks in one call");
    uint8_t* d_slots; int64_t* d_size; int64_t* d_off = d_comp_off;
    SL_TRY(scratch("bgzf.deflate.slots", static_cast<size_t>(n_blocks) * DF_SLOT, &d_slots));
    SL_TRY(scratch("bgzf.deflate.size", static_cast<size_t>(n_blocks) + 1, &d_size));
    if (!d_off) SL_TRY(scratch("bgzf.deflate.off", static_cast<size_t>(n_blocks) + 1, &d_off));
    SL_HIP(hipMemsetAsync(d_size + n_blocks, 0, sizeof(int64_t), s));
    Context& c = ctx();
    SL_HIP(hipEventRecord(c.ev_start, s));
    const auto kernel = use_cuts ? k_bgzf_deflate<true> : k_bgzf_deflate<false>;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(n_blocks)), dim3(64), 0, s, d_text, static_cast<long long>(nbytes), static_cast<long long>(n_blocks), mode, d_cuts,
                       static_cast<long long>(n_cuts), static_cast<long long>(cut_origin), d_slots, d_size);
    SL_HIP(hipGetLastError());
    SL_HIP(hipEventRecord(c.ev_stop, s));
    c.timed = true;
    SL_TRY(exclusive_scan("bgzf.deflate.scan", d_size, d_off, static_cast<size_t>(n_blocks) + 1, s));
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>((need / 16 + 255) / 256, static_cast<int64_t>(c.num_cu) * 32));
    hipLaunchKernelGGL(k_bgzf_pack, dim3(grid), dim3(256), 0, s, d_slots, d_off, static_cast<long long>(n_blocks), d_comp);
    SL_HIP(hipGetLastError());
    int64_t total = 0;
    SL_HIP(hipMemcpyAsync(&total, d_off + n_blocks, sizeof total, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    *comp_bytes = total;
    return 0;
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_bgzf_deflate_bound(int64_t nbytes, int64_t* n_blocks, int64_t* comp_capacity) {
    return bgzf_deflate_bound(nbytes, n_blocks, comp_capacity);
}

int sarlacc_dev_bgzf_deflate(const uint8_t* d_text, int64_t nbytes, int mode, uint8_t* d_comp, int64_t comp_capacity,
                             int64_t* d_comp_off, int64_t* comp_bytes, void* stream) {
    return bgzf_deflate(d_text, nbytes, false, nullptr, 0, 0, mode, d_comp, comp_capacity, d_comp_off, comp_bytes,
                        static_cast<hipStream_t>(stream));
}

int sarlacc_dev_bgzf_deflate_cuts(const uint8_t* d_text, int64_t nbytes, const int64_t* d_cuts, int64_t n_cuts,
                                  int64_t cut_origin, int mode, uint8_t* d_comp, int64_t comp_capacity,
                                  int64_t* d_comp_off, int64_t* comp_bytes, void* stream) {
    return bgzf_deflate(d_text, nbytes, true, d_cuts, n_cuts, cut_origin, mode, d_comp, comp_capacity, d_comp_off, comp_bytes,
                        static_cast<hipStream_t>(stream));
}
}
