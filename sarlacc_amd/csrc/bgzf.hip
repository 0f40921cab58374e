// bgzf.hip -- BGZF (blocked gzip, SAM specification section 4.1; RFC 1951 / RFC 1952) on gfx950: the host walks the
// block headers, the device inflates the blocks into text that the FASTQ and SAM parsers read where it lies.
//
//   sarlacc_bgzf_scan         host: offsets and inflated sizes of the complete blocks of a piece of a file
//   k_bgzf_inflate            one wavefront per BGZF block (one 64-thread workgroup each, assigned statically)
//   k_bgzf_crc                one wavefront per BGZF block: CRC-32 of its output against the trailer
//   k_copy_bytes              device-to-device carry-over of a text tail (sarlacc_dev_copy)
//   k_rfind_byte              position of the last occurrence of a byte (sarlacc_dev_rfind_byte)
//
// k_bgzf_inflate.  Symbol decoding is serial: lane 0 walks the bit stream through a 1-KB window of the compressed
// bytes in LDS (refilled by all lanes) and the decode tables of the current deflate block in LDS, and fills a queue
// of up to 64 tokens (a literal, or a length and a distance).  Then the whole wavefront writes the batch: a prefix
// sum over the token lengths gives every token its place, and the lanes walk the batch's bytes 64 at a time.  The
// byte at output position q belongs to one token (binary search over the 64 starts); a literal's value stands in
// the queue; a match byte is the byte at  start - dist + (q - start) % dist,  which lies before the token's start,
// so following it leads to an earlier token of the batch (at most 63 hops) or to a byte that an earlier batch wrote.
// That makes overlapping copies (dist < length, dist < 64) and matches fed by the same batch exact without any
// order among the lanes.  History is read back from the wavefront's own global stores: every batch ends with a
// workgroup-scope fence (the stores have completed before a later load is issued; the CU's L1 is coherent for
// its own wavefronts).  The alternative, a 32-KB LDS ring per wavefront, would hold a CU to four wavefronts; the
// ~5 KB used here leave the wavefront limit to the registers.  Neither has been measured against the other.
//
// Bounds (a compressed file is untrusted): the window is filled with zeros beyond the block's payload, and a token
// whose bits end beyond the payload is "compressed data ends early", so the bit reader touches nothing past the
// payload and never the trailer; a token is queued only if its bytes fit in text_off[k+1] - text_off[k]; a distance
// beyond the bytes produced is refused; code lengths are checked (Kraft sum) before a table is filled; every loop
// advances the bit position or the output position, both bounded by the block's sizes.  No spin-wait, no
// dependence between workgroups, no printf/assert.
#include "common.hpp"
#include "crc32.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <cstdlib>

namespace sarlacc {
namespace {

typedef uint32_t __attribute__((aligned(1))) u32_any;

enum {
    BZ_OK = 0, BZ_STORED = 1, BZ_LENGTHS = 2, BZ_SYMBOL = 3, BZ_DISTANCE = 4, BZ_OVERFLOW = 5, BZ_EARLY = 6, BZ_LENGTH = 7,
    BZ_CRC = 8
};
const char* const BZ_REASON[] = {"", "invalid stored block", "invalid code lengths", "invalid symbol",
                                 "distance beyond the start of the block", "output exceeds the size field",
                                 "compressed data ends early", "length mismatch", "CRC32 mismatch"};

constexpr int WIN_BYTES = 1024;          // window of compressed bytes: 16 per lane
constexpr int WIN_WORDS = WIN_BYTES / 4;
constexpr int LIT_BITS = 10, DIST_BITS = 8;
constexpr int MAX_TOKEN_BITS = 48;       // 15 + 5 + 15 + 13
constexpr int MAX_BLOCK = 65536;

__constant__ uint16_t c_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                                        131, 163, 195, 227, 258};
__constant__ uint8_t c_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                         2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one canonical Huffman code in LDS: a direct table over the first BITS bits (entry = symbol << 4 | length, 0 = longer
// or none) and, for the longer codes, the counts / sorted symbols of the bit-by-bit walk
template <int NSYM, int BITS>
struct Huff {
    uint16_t fast[1 << BITS];
    uint16_t sorted[NSYM];
    uint16_t count[16];     // codes per length
    uint16_t first[16];     // index in sorted[] of the first symbol of a length
    uint16_t code0[16];     // canonical code of that symbol
    uint16_t next[16];      // huff_prepare's running place per length
};

struct Shared {
    uint32_t win[WIN_WORDS + 2];
    uint8_t lens[320];
    Huff<288, LIT_BITS> lit;
    Huff<32, DIST_BITS> dist;
    Huff<19, 7> clen;
    uint16_t tok_len[64];      // bytes of the token (1: literal)
    uint16_t tok_val[64];      // literal value, or distance
    uint16_t tok_start[65];    // start of the token in the batch
    int uni[4];                // lane 0 -> wavefront: what the last serial phase left
};

__device__ __forceinline__ void fence_wave() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// Window of the payload bytes from `wbyte` on, zeros beyond `nbytes`.  All lanes.
__device__ __forceinline__ void fill_window(Shared& sh, const uint8_t* pay, int nbytes, int wbyte, int lane) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int w = lane + 64 * k, b = wbyte + 4 * w;
        uint32_t v = 0;
        if (b + 4 <= nbytes) v = *reinterpret_cast<const u32_any*>(pay + b);
        else
            for (int j = 0; j < 4; ++j)
                if (b + j < nbytes) v |= static_cast<uint32_t>(pay[b + j]) << (8 * j);
        sh.win[w] = v;
    }
    if (lane < 2) sh.win[WIN_WORDS + lane] = 0;
    fence_wave();
}

// 32 bits of the window from window bit `wp` (wp <= 32 * WIN_WORDS)
__device__ __forceinline__ uint32_t peek(const Shared& sh, int wp) {
    const int i = wp >> 5;
    const uint64_t v = (static_cast<uint64_t>(sh.win[i + 1]) << 32) | sh.win[i];
    return static_cast<uint32_t>(v >> (wp & 31));
}

// Counts, Kraft check, sorted symbols of `n` code lengths (lane 0).  An over-subscribed code is refused, and an
// incomplete one as zlib refuses it: a literal/length or distance code may be a single code of 1 bit, a distance
// code may be absent (a block of literals only), and the code-length code (NSYM == 19) is never incomplete -- after
// a lone code-length code all lengths would be equal, and 257 to 286 equal lengths are no complete code.  Returns 0
// or BZ_LENGTHS; count[0] is left holding the number of symbols that have a code.
template <int NSYM, int BITS>
__device__ int huff_prepare(Huff<NSYM, BITS>& h, const uint8_t* lens, int n) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int s = 0; s < n; ++s) h.count[lens[s]]++;
    int left = 1, used = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - h.count[l];
        if (left < 0) return BZ_LENGTHS;             // over-subscribed
        used += h.count[l];
    }
    if (left > 0) {                                  // incomplete
        const bool lone = used == 1 && h.count[1] == 1, absent = used == 0 && NSYM == 32;
        if (NSYM == 19 || !(lone || absent)) return BZ_LENGTHS;
    }
    int idx = 0, code = 0;
    for (int l = 1; l < 16; ++l) {
        h.first[l] = static_cast<uint16_t>(idx);
        h.code0[l] = static_cast<uint16_t>(code);
        h.next[l] = static_cast<uint16_t>(idx);
        idx += h.count[l];
        code = (code + h.count[l]) << 1;
    }
    for (int s = 0; s < n; ++s)
        if (lens[s]) h.sorted[h.next[lens[s]]++] = static_cast<uint16_t>(s);
    h.count[0] = static_cast<uint16_t>(used);
    return 0;
}

// Direct table from the prepared code.  All lanes.
template <int NSYM, int BITS>
__device__ void huff_fill(Huff<NSYM, BITS>& h, const uint8_t* lens, int lane) {
    for (int e = lane; e < (1 << BITS); e += 64) h.fast[e] = 0;
    fence_wave();
    const int used = h.count[0];
    for (int i = lane; i < used; i += 64) {
        const int s = h.sorted[i], l = lens[s];
        if (l > BITS) continue;
        const uint32_t code = h.code0[l] + (i - h.first[l]);
        const uint32_t rev = __brev(code) >> (32 - l);
        const uint16_t entry = static_cast<uint16_t>((s << 4) | l);
        for (uint32_t e = rev; e < (1u << BITS); e += 1u << l) h.fast[e] = entry;
    }
    fence_wave();
}

// One symbol from the bits `v` (LSB first).  Returns the symbol and its length in *len; -1: no such code (15 bits).
template <int NSYM, int BITS>
__device__ __forceinline__ int huff_decode(const Huff<NSYM, BITS>& h, uint32_t v, int* len) {
    const uint16_t e = h.fast[v & ((1u << BITS) - 1)];
    if (e) {
        *len = e & 15;
        return e >> 4;
    }
    int code = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code << 1) | static_cast<int>((v >> (l - 1)) & 1u);
        const int k = code - h.code0[l];
        if (k >= 0 && k < h.count[l]) {
            *len = l;
            return h.sorted[h.first[l] + k];
        }
    }
    *len = 15;
    return -1;
}

// (CRC-32: crc_mul, crc_shift and crc_table_entry are in crc32.hpp)
__device__ __forceinline__ uint32_t le32(const uint8_t* p) {
    return p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
}

// Header of block k as it lies in the file: payload start and size.  False: the sizes do not hold a block.
__device__ __forceinline__ bool block_frame(const uint8_t* blk, long long csize, int* hdr, int* pay_bytes) {
    if (csize < 12 + 8 || csize > MAX_BLOCK) return false;
    const int xlen = blk[10] | (blk[11] << 8);
    *hdr = 12 + xlen;
    if (*hdr + 8 > csize) return false;
    *pay_bytes = static_cast<int>(csize) - *hdr - 8;
    return true;
}

__global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_off,
                                                     const int64_t* __restrict__ text_off, long long nblocks, uint8_t* text,
                                                     int check_size, int* __restrict__ status) {
    __shared__ Shared sh;
    const long long k = blockIdx.x;
    if (k >= nblocks) return;
    const int lane = threadIdx.x;
    const uint8_t* blk = comp + comp_off[k];
    const long long csize = comp_off[k + 1] - comp_off[k];
    const long long want = text_off[k + 1] - text_off[k];
    uint8_t* out = text + text_off[k];
    int hdr = 0, pay_bytes = 0;
    int err = 0;
    if (!block_frame(blk, csize, &hdr, &pay_bytes)) err = BZ_EARLY;
    else if (want < 0 || want > MAX_BLOCK) err = BZ_LENGTH;
    else if (check_size && le32(blk + csize - 4) != static_cast<uint32_t>(want)) err = BZ_LENGTH;
    if (err) {
        if (lane == 0) status[k] = err;
        return;
    }
    const uint8_t* pay = blk + hdr;
    const int end_bits = pay_bytes * 8;
    const int cap = static_cast<int>(want);
    int pos = 0;          // bit position in the payload (uniform)
    int produced = 0;     // bytes written (uniform)
    bool last = false;

    // every deflate block takes at least 3 bits: the loop ends with the payload
    while (!last && !err) {
        fill_window(sh, pay, pay_bytes, pos >> 3, lane);
        int wp = pos & 7;                     // bit in the window
        const int wbase = (pos >> 3) * 8;     // payload bit of window bit 0
        uint32_t v = peek(sh, wp);
        if (pos + 3 > end_bits) { err = BZ_EARLY; break; }
        last = v & 1u;
        const int type = (v >> 1) & 3;
        wp += 3;
        if (type == 3) { err = BZ_STORED; break; }
        if (type == 0) {
            wp = (wp + 7) & ~7;
            if (wbase + wp + 32 > end_bits) { err = BZ_EARLY; break; }
            v = peek(sh, wp);
            const int len = v & 0xffffu;
            if ((len ^ 0xffffu) != static_cast<int>(v >> 16)) { err = BZ_STORED; break; }
            const int src = (wbase + wp + 32) >> 3;
            if (src + len > pay_bytes) { err = BZ_EARLY; break; }
            if (produced + len > cap) { err = BZ_OVERFLOW; break; }
            for (int i = lane; i < len; i += 64) out[produced + i] = pay[src + i];
            fence_wave();
            produced += len;
            pos = (src + len) * 8;
            continue;
        }
        pos = wbase + wp;
        if (type == 1) {
            for (int s = lane; s < 320; s += 64) sh.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            fence_wave();
            if (lane == 0) {
                huff_prepare(sh.lit, sh.lens, 288);
                huff_prepare(sh.dist, sh.lens + 288, 32);   // 5 bits flat; symbols 30 and 31 are refused when they are met
            }
            fence_wave();
            huff_fill(sh.lit, sh.lens, lane);
            huff_fill(sh.dist, sh.lens + 288, lane);
        } else {
            // code lengths: at most 14 + 57 + 320 * 14 bits = 569 bytes, inside one window
            int nlen = 0, ndist = 0;
            if (lane == 0) {
                int e = 0;
                v = peek(sh, wp);
                nlen = (v & 31) + 257;
                ndist = ((v >> 5) & 31) + 1;
                const int ncode = ((v >> 10) & 15) + 4;
                wp += 14;
                if (nlen > 286 || ndist > 30) e = BZ_LENGTHS;
                for (int i = 0; i < 19; ++i) sh.lens[i] = 0;
                for (int i = 0; i < ncode; ++i) {
                    sh.lens[c_clen_order[i]] = peek(sh, wp) & 7;
                    wp += 3;
                }
                if (!e) e = huff_prepare(sh.clen, sh.lens, 19);
                if (!e && sh.clen.count[0] == 0) e = BZ_LENGTHS;
                if (!e) {
                    // direct table of the (at most 7-bit) code-length code, serially: 128 entries
                    for (int i = 0; i < 128; ++i) sh.clen.fast[i] = 0;
                    const int used = sh.clen.count[0];
                    for (int i = 0; i < used; ++i) {
                        const int s = sh.clen.sorted[i], l = sh.lens[s];
                        const uint32_t code = sh.clen.code0[l] + (i - sh.clen.first[l]);
                        const uint32_t rev = __brev(code) >> (32 - l);
                        for (uint32_t t = rev; t < 128u; t += 1u << l) sh.clen.fast[t] = static_cast<uint16_t>((s << 4) | l);
                    }
                    int idx = 0;
                    const int total = nlen + ndist;
                    while (idx < total && !e) {      // every turn adds at least one length
                        v = peek(sh, wp);
                        int l;
                        const int s = huff_decode(sh.clen, v, &l);
                        if (s < 0) { e = wbase + wp + 7 > end_bits ? BZ_EARLY : BZ_LENGTHS; break; }
                        wp += l;
                        v >>= l;
                        if (s < 16) {
                            sh.lens[idx++] = static_cast<uint8_t>(s);
                        } else {
                            int rep, val = 0;
                            if (s == 16) {
                                if (idx == 0) { e = BZ_LENGTHS; break; }
                                val = sh.lens[idx - 1];
                                rep = 3 + (v & 3); wp += 2;
                            } else if (s == 17) {
                                rep = 3 + (v & 7); wp += 3;
                            } else {
                                rep = 11 + (v & 127); wp += 7;
                            }
                            if (idx + rep > total) { e = BZ_LENGTHS; break; }
                            for (int r = 0; r < rep; ++r) sh.lens[idx++] = static_cast<uint8_t>(val);
                        }
                    }
                }
                if (wbase + wp > end_bits) e = BZ_EARLY;
                if (!e && sh.lens[256] == 0) e = BZ_LENGTHS;      // no end-of-block code
                if (!e) {
                    // the two codes side by side at fixed places: literal/length at 0, distance at 288
                    for (int i = ndist - 1; i >= 0; --i) sh.lens[288 + i] = sh.lens[nlen + i];
                    for (int i = nlen; i < 288; ++i) sh.lens[i] = 0;
                    for (int i = 288 + ndist; i < 320; ++i) sh.lens[i] = 0;
                    e = huff_prepare(sh.lit, sh.lens, 288);
                    if (!e) e = huff_prepare(sh.dist, sh.lens + 288, 32);
                }
                sh.uni[0] = e;
                sh.uni[1] = wbase + wp;
            }
            fence_wave();
            err = sh.uni[0];
            pos = sh.uni[1];
            if (err) break;
            huff_fill(sh.lit, sh.lens, lane);
            huff_fill(sh.dist, sh.lens + 288, lane);
        }

        // tokens of this deflate block, a batch at a time; every batch consumes bits or ends the block
        bool eob = false;
        while (!eob && !err) {
            fill_window(sh, pay, pay_bytes, pos >> 3, lane);
            if (lane == 0) {
                int wq = pos & 7;
                const int wb = (pos >> 3) * 8;
                int n = 0, bytes = 0, e = 0, done = 0;
                while (n < 64 && wq + MAX_TOKEN_BITS <= WIN_BYTES * 8) {
                    uint32_t b = peek(sh, wq);
                    int l;
                    int s = huff_decode(sh.lit, b, &l);
                    int q = wq + l;
                    if (s < 0) { e = wb + q > end_bits ? BZ_EARLY : BZ_SYMBOL; break; }
                    if (s < 256) {
                        if (wb + q > end_bits) { e = BZ_EARLY; break; }
                        if (produced + bytes + 1 > cap) { e = BZ_OVERFLOW; break; }
                        sh.tok_len[n] = 1;
                        sh.tok_val[n] = static_cast<uint16_t>(s);
                        bytes += 1; ++n; wq = q;
                        continue;
                    }
                    if (s == 256) {
                        if (wb + q > end_bits) { e = BZ_EARLY; break; }
                        wq = q; done = 1;
                        break;
                    }
                    s -= 257;
                    if (s >= 29) { e = wb + q > end_bits ? BZ_EARLY : BZ_SYMBOL; break; }
                    b >>= l;
                    const int xl = c_len_extra[s];
                    const int mlen = c_len_base[s] + static_cast<int>(b & ((1u << xl) - 1));
                    q += xl;
                    b = peek(sh, q);
                    int d = huff_decode(sh.dist, b, &l);
                    q += l;
                    if (d < 0 || d >= 30) { e = wb + q > end_bits ? BZ_EARLY : BZ_SYMBOL; break; }
                    b >>= l;
                    const int xd = c_dist_extra[d];
                    const int dist = c_dist_base[d] + static_cast<int>(b & ((1u << xd) - 1));
                    q += xd;
                    if (wb + q > end_bits) { e = BZ_EARLY; break; }
                    if (dist > produced + bytes) { e = BZ_DISTANCE; break; }
                    if (produced + bytes + mlen > cap) { e = BZ_OVERFLOW; break; }
                    sh.tok_len[n] = static_cast<uint16_t>(mlen);
                    sh.tok_val[n] = static_cast<uint16_t>(dist);
                    bytes += mlen; ++n; wq = q;
                }
                sh.uni[0] = e;
                sh.uni[1] = wb + wq;
                sh.uni[2] = n;
                sh.uni[3] = done;
            }
            fence_wave();
            err = sh.uni[0];
            pos = sh.uni[1];
            const int ntok = sh.uni[2];
            eob = sh.uni[3] != 0;
            // the tokens decoded before an error are not written: the block is refused as a whole
            if (err) break;
            // place of every token in the batch
            const int mylen = lane < ntok ? sh.tok_len[lane] : 0;
            int incl = mylen;
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            sh.tok_start[lane] = static_cast<uint16_t>(incl - mylen);
            const int total = __shfl(incl, 63);
            if (lane == 63) sh.tok_start[64] = static_cast<uint16_t>(total);   // at most 64 * 258
            fence_wave();
            for (int i = lane; i < total; i += 64) {
                // the token that holds byte i: the last one that starts at or before it (empty slots start at `total`)
                int t = 0;
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (t + step < ntok && sh.tok_start[t + step] <= i) t += step;
                int q = i;            // byte of the batch whose value byte i takes
                int value = -1;
                long long src = 0;    // or the byte of the block's output
                for (int hop = 0; hop < 64; ++hop) {
                    const int st = sh.tok_start[t];
                    if (sh.tok_len[t] == 1) { value = sh.tok_val[t]; break; }
                    const int d = sh.tok_val[t];
                    int r = q - st;
                    if (r >= d) r %= d;
                    q = st - d + r;                  // before the token's start
                    if (q < 0) { src = produced + q; break; }   // (>= 0: the decoder checked the distance)
                    // the earlier token that holds q
                    int u = 0;
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1)
                        if (u + step < t && sh.tok_start[u + step] <= q) u += step;
                    t = u;
                }
                if (value < 0) value = out[src];
                out[produced + i] = static_cast<uint8_t>(value);
            }
            fence_wave();
            produced += total;
        }
    }
    if (!err && produced != cap) err = BZ_LENGTH;
    if (lane == 0) status[k] = err;
}

// CRC-32 of every block's output against its trailer: the lanes take equal slices, the slices' CRCs are shifted to
// the end of the block and folded (crc(A B) = crc(A) x^(8 |B|) + crc(B)).  Blocks that failed before are left alone.
__global__ void __launch_bounds__(64) k_bgzf_crc(const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_off,
                                                 const int64_t* __restrict__ text_off, long long nblocks,
                                                 const uint8_t* __restrict__ text, int* status) {
    __shared__ uint32_t table[256];
    const long long k = blockIdx.x;
    if (k >= nblocks) return;
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) table[i] = crc_table_entry(i);
    __syncthreads();
    if (status[k] != 0) return;
    const long long csize = comp_off[k + 1] - comp_off[k];
    const int n = static_cast<int>(text_off[k + 1] - text_off[k]);    // 0 .. 65536: k_bgzf_inflate checked it
    const uint8_t* p = text + text_off[k];
    const int slice = (n + 63) / 64;
    const int b = min(lane * slice, n), e = min(b + slice, n);
    uint32_t c = 0xffffffffu;
    for (int i = b; i < e; ++i) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    c = e > b ? ~c : 0u;                               // an empty slice adds nothing
    c = crc_shift(c, static_cast<uint32_t>(n - e));
    for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o);
    if (lane == 0 && c != le32(comp + comp_off[k] + csize - 8)) status[k] = BZ_CRC;
}

__global__ void k_copy_bytes(uint8_t* dst, const uint8_t* src, long long n) {
    for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * blockDim.x)
        dst[i] = src[i];
}

__global__ void k_rfind_byte(const uint8_t* text, long long n, int value, long long* out) {
    long long best = -1;
    for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * blockDim.x)
        if (text[i] == value) best = i;
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0 && best >= 0) atomicMax(out, best);
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

int sarlacc_bgzf_scan(const uint8_t* buf, int64_t nbytes, int64_t max_blocks, int64_t first_block, int64_t* comp_off,
                      int64_t* text_off, int64_t* n_blocks, int64_t* used_bytes, int* last_is_eof) {
    if (nbytes < 0 || max_blocks < 0) return fail("sarlacc_amd: negative BGZF size");
    int64_t n = 0, o = 0, t = 0;
    int eof = 0;
    comp_off[0] = 0;
    text_off[0] = 0;
    while (n < max_blocks && o < nbytes) {
        const uint8_t* p = buf + o;
        const int64_t r = nbytes - o;
        const long long K = static_cast<long long>(first_block + n + 1);
        if ((r >= 1 && p[0] != 0x1f) || (r >= 2 && p[1] != 0x8b) || (r >= 3 && p[2] != 8))
            return fail("BGZF block %lld: not a gzip member", K);
        if (r >= 4 && !(p[3] & 4)) return fail("BGZF block %lld: no BC subfield", K);
        if (r < 12) break;
        const int64_t xlen = p[10] | (p[11] << 8);
        if (r < 12 + xlen) break;
        int64_t bsize = -1;
        for (int64_t f = 12; f + 4 <= 12 + xlen;) {
            const int64_t slen = p[f + 2] | (p[f + 3] << 8);
            if (f + 4 + slen > 12 + xlen) break;
            if (p[f] == 'B' && p[f + 1] == 'C' && slen == 2) {
                bsize = p[f + 4] | (p[f + 5] << 8);
                break;
            }
            f += 4 + slen;
        }
        if (bsize < 0) return fail("BGZF block %lld: no BC subfield", K);
        const int64_t total = bsize + 1;
        if (total < 12 + xlen + 8) return fail("BGZF block %lld: block size field is inconsistent", K);
        if (r < total) break;
        const uint8_t* q = p + total - 4;
        const int64_t isize = static_cast<int64_t>(q[0]) | (static_cast<int64_t>(q[1]) << 8) | (static_cast<int64_t>(q[2]) << 16) |
                              (static_cast<int64_t>(q[3]) << 24);
        if (isize > 65536) return fail("BGZF block %lld: uncompressed size exceeds 65536", K);
        eof = total == 28 && isize == 0;
        o += total;
        t += isize;
        ++n;
        comp_off[n] = o;
        text_off[n] = t;
    }
    *n_blocks = n;
    *used_bytes = o;
    *last_is_eof = n > 0 ? eof : 0;
    return 0;
}

int sarlacc_dev_bgzf_inflate(const uint8_t* d_comp, const int64_t* d_comp_off, const int64_t* d_text_off, int64_t n_blocks,
                             int64_t first_block, uint8_t* d_text, int check_crc, void* stream) {
    SL_TRY(ensure_device());
    if (n_blocks < 0) return fail("sarlacc_amd: negative BGZF block count");
    if (n_blocks == 0) return 0;
    if (n_blocks > 0x7fffffffLL) return fail("sarlacc_amd: more than 2^31 - 1 BGZF blocks in one call");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int* d_status;
    SL_TRY(scratch("bgzf.status", static_cast<size_t>(n_blocks), &d_status));
    SL_HIP(hipMemsetAsync(d_status, 0, sizeof(int) * static_cast<size_t>(n_blocks), s));
    Context& c = ctx();
    SL_HIP(hipEventRecord(c.ev_start, s));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(static_cast<unsigned>(n_blocks)), dim3(64), 0, s, d_comp, d_comp_off, d_text_off,
                       static_cast<long long>(n_blocks), d_text, check_crc ? 1 : 0, d_status);
    SL_HIP(hipGetLastError());
    SL_HIP(hipEventRecord(c.ev_stop, s));
    c.timed = true;
    if (check_crc) {
        hipLaunchKernelGGL(k_bgzf_crc, dim3(static_cast<unsigned>(n_blocks)), dim3(64), 0, s, d_comp, d_comp_off, d_text_off,
                           static_cast<long long>(n_blocks), d_text, d_status);
        SL_HIP(hipGetLastError());
    }
    std::vector<int> status(static_cast<size_t>(n_blocks));
    SL_HIP(hipMemcpyAsync(status.data(), d_status, sizeof(int) * status.size(), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    for (int64_t k = 0; k < n_blocks; ++k) {
        const int e = status[static_cast<size_t>(k)];
        if (e) return fail("BGZF block %lld: %s", static_cast<long long>(first_block + k + 1), BZ_REASON[e >= 0 && e <= BZ_CRC ? e : BZ_SYMBOL]);
    }
    return 0;
}

int sarlacc_dev_copy(void* d_dst, const void* d_src, int64_t bytes, void* stream) {
    SL_TRY(ensure_device());
    if (bytes < 0) return fail("sarlacc_amd: negative copy size");
    if (bytes == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>((bytes + 255) / 256, static_cast<int64_t>(ctx().num_cu) * 32));
    hipLaunchKernelGGL(k_copy_bytes, dim3(grid), dim3(256), 0, s, static_cast<uint8_t*>(d_dst), static_cast<const uint8_t*>(d_src),
                       static_cast<long long>(bytes));
    SL_HIP(hipGetLastError());
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

int sarlacc_dev_rfind_byte(const uint8_t* d_text, int64_t nbytes, int value, int64_t* pos, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0) return fail("sarlacc_amd: negative text size");
    *pos = -1;
    if (nbytes == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long* d_pos;
    SL_TRY(scratch("bgzf.rfind", 1, &d_pos));
    SL_HIP(hipMemsetAsync(d_pos, 0xff, sizeof(long long), s));
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>((nbytes + 255) / 256, static_cast<int64_t>(ctx().num_cu) * 32));
    hipLaunchKernelGGL(k_rfind_byte, dim3(grid), dim3(256), 0, s, d_text, static_cast<long long>(nbytes), value & 0xff, d_pos);
    SL_HIP(hipGetLastError());
    long long p = -1;
    SL_HIP(hipMemcpyAsync(&p, d_pos, sizeof p, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    *pos = p;
    return 0;
}
}
