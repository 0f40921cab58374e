// bam.hip -- BAM alignment records -> ranges, on gfx950 (sam2ranges on the binary form of a SAM file; SAM specification
// section 4.2).  The caller inflates the BGZF blocks on the device (bgzf.hip) and reads the header on the host; this file
// gets nbytes of inflated BAM whose byte 0 is the start of a record.
//
// A record is block_size (int32, little-endian, any alignment) followed by block_size bytes, so the start of record
// i + 1 is known only through record i.  The locator finds every start exactly -- each one is reached from byte 0 through
// size fields alone, nothing is accepted because it looks like a record -- without a one-lane walk over the records:
//
//   k_bam_hops     one workgroup per tile of BAM_TILE bytes.  An LDS table of one 32-bit entry per byte: entry e starts as
//                  e + 4 + block_size(e), where the record that would start at e ends, relative to the tile; HOP_INVALID
//                  for a block_size below 32, HOP_PARTIAL for a size field that is not wholly inside the buffer.  Pointer
//                  jumping, hop[e] = hop[hop[e]] while hop[e] < BAM_TILE, at most BAM_ROUNDS rounds (a record is at least
//                  36 bytes, so a chain holds at most BAM_TILE / 36 + 1 starts; a round at least doubles the steps an entry
//                  spans), stopped early when every entry has left the tile.  Afterwards every entry holds where the
//                  chain that enters the tile at that byte leaves it.  The table goes to HBM, 4 bytes per byte of input.
//   k_bam_chain    one wavefront: from byte 0, one table look-up per tile that a record starts in; it marks each such
//                  tile's entry offset.  nbytes / BAM_TILE dependent loads instead of one per record.
//   k_bam_starts   one lane per tile with an entry walks the tile's starts from the entry, reading the size fields again:
//                  first to count them (rocPRIM exclusive scan over the tiles), then to write rec_off.  The tile in which
//                  the chain ends reports how: the end of the buffer, an incomplete record, or a block_size below 32.
//   k_bam_fields   one wavefront per record: the fixed fields, the keep decision, and on kept records the CIGAR array
//                  (lanes stride over the ops; a 64-bit wave reduction sums the reference-consuming lengths).  A kept record
//                  whose CIGAR is the stand-in <l_seq>S<n>N of a CIGAR above 65 535 ops has its tags walked by one lane
//                  for the CG:B,I array.  It fills SamRec / keep / name_len as k_sam_fields does; the scans and the
//                  extract step are shared with the SAM reader (ranges_index, k_sam_scatter).
//
// The host side is in readers_host.cpp: the locator's launch sequence (bam_locate, which bam_reads.hip's records go
// through as well), the entry points and the messages below.  The functions at the end of this file only enqueue.  The
// layout check is bam_layout_ok (bam_rec.hpp).
//
// No kernel waits on a value another workgroup writes: the launches are the synchronisation.  Every loop is bounded by
// BAM_TILE or nbytes, no byte at or beyond nbytes is read, and a bad file is an error return (the first_bad pattern of
// k_sam_fields: atomicMin on (record << 4 | code)), never a fault.
//
// Messages, "BAM record K: <reason>", K 1-based over the alignment records of the file:
//   locator      file ends inside the record | block size below 32
//   layout       record fields do not fit its block size
//   pos          POS is not a 32-bit integer
//   rname        reference ID outside the header's reference list
//   cigar_star   no CIGAR on a kept record
//   cigar_op     CIGAR operation code above 8
//   tags         malformed tags or CG tag behind a long-CIGAR stand-in
//   cigar_range  CIGAR length above 2^31 - 1
//   cigar_clips  CIGAR has only H and S operations
//   end          alignment end outside the 32-bit integer range
#include "bam_rec.hpp"
#include "devprim.hpp"
#include "readers.hpp"

#include <algorithm>
#include <climits>

namespace sarlacc {

constexpr int BAM_HOP_THREADS = 1024;
constexpr int BAM_MIN_RECORD = 36;               // block_size + the 32 fixed bytes
constexpr int BAM_MAX_STARTS = (BAM_TILE + BAM_MIN_RECORD - 1) / BAM_MIN_RECORD;   // 456 starts of one chain in a tile
constexpr int BAM_ROUNDS = 10;                   // ceil(log2(456)) = 9 rounds resolve every entry, one more sees no change
constexpr unsigned HOP_INVALID = 0xffffffffu;    // block_size below 32
constexpr unsigned HOP_PARTIAL = 0xfffffffeu;    // size field not wholly inside the buffer
static_assert((1 << (BAM_ROUNDS - 1)) >= BAM_MAX_STARTS, "pointer jumping needs more rounds for this tile");
static_assert(BAM_TILE % (4 * BAM_HOP_THREADS) == 0, "the fill takes four entries per thread and step");

__global__ void __launch_bounds__(BAM_HOP_THREADS) k_bam_hops(const uint8_t* bam, long long nbytes, unsigned* table) {
    __shared__ unsigned hop[BAM_TILE];
    const long long t0 = static_cast<long long>(blockIdx.x) * BAM_TILE;
    const int n = static_cast<int>(std::min<long long>(BAM_TILE, nbytes - t0));
    // four entries per thread and step from the seven bytes they cover
    for (int e = threadIdx.x * 4; e < BAM_TILE; e += 4 * BAM_HOP_THREADS) {
        unsigned long long w = 0;
        for (int j = 0; j < 7; ++j) {
            const long long p = t0 + e + j;
            if (p < nbytes) w |= static_cast<unsigned long long>(bam[p]) << (8 * j);
        }
        unsigned v[4];
        for (int i = 0; i < 4; ++i) {
            if (t0 + e + i + 4 > nbytes) {
                v[i] = HOP_PARTIAL;
            } else {
                const int bs = static_cast<int>(static_cast<unsigned>(w >> (8 * i)));
                v[i] = bs < 32 ? HOP_INVALID : static_cast<unsigned>(e + i + 4) + static_cast<unsigned>(bs);
            }
        }
        *reinterpret_cast<uint4*>(&hop[e]) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    // a racing read of hop[h] sees the old or the new value; both lie on the chain of e, at or beyond the old one
    for (int r = 0; r < BAM_ROUNDS; ++r) {
        int changed = 0;
        for (int e = threadIdx.x; e < BAM_TILE; e += BAM_HOP_THREADS) {
            const unsigned h = hop[e];
            if (h < static_cast<unsigned>(BAM_TILE)) {
                hop[e] = hop[h];
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    for (int e = threadIdx.x; e < n; e += BAM_HOP_THREADS) table[t0 + e] = hop[e];
}

// entry[tile] = offset of the first record that starts in the tile (left at -1 where none does)
__global__ void __launch_bounds__(64) k_bam_chain(const unsigned* table, long long nbytes, long long ntiles, long long* entry) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long s = 0;
    for (long long it = 0; it < ntiles && s < nbytes; ++it) {      // every step lands in a later tile
        const long long tile = s / BAM_TILE;
        entry[tile] = s;
        const unsigned x = table[s];
        if (x >= HOP_PARTIAL || x < static_cast<unsigned>(BAM_TILE)) break;
        s = tile * BAM_TILE + x;
    }
}

// WRITE = false: count[tile] = complete records that start in the tile, and the tile in which the chain ends writes
// term = (offset of the first record that is not wholly in the buffer, BAM_CHAIN_*).  WRITE = true: their offsets.
template <bool WRITE>
__global__ void __launch_bounds__(64) k_bam_starts(const uint8_t* bam, long long nbytes, long long ntiles, const long long* entry,
                                                   long long* count, const long long* base, long long* rec_off, long long* term) {
    const long long tile = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
    if (tile >= ntiles) return;
    long long s = entry[tile];
    if (s < 0) {
        if (!WRITE) count[tile] = 0;
        return;
    }
    const long long tile_end = (tile + 1) * BAM_TILE;
    long long n = 0;
    int code = BAM_CHAIN_CLEAN;
    for (int i = 0; i < BAM_MAX_STARTS && s < tile_end && s < nbytes; ++i) {
        if (s + 4 > nbytes) { code = BAM_CHAIN_INCOMPLETE; break; }
        const int bs = static_cast<int>(rd_u32(bam + s));
        if (bs < 32) { code = BAM_CHAIN_SIZE; break; }
        if (s + 4 + bs > nbytes) { code = BAM_CHAIN_INCOMPLETE; break; }
        if (WRITE) rec_off[base[tile] + n] = s;
        ++n;
        s += 4 + static_cast<long long>(bs);
    }
    if (!WRITE) {
        count[tile] = n;
        if (code != BAM_CHAIN_CLEAN || s == nbytes) {
            term[0] = s;
            term[1] = code;
        }
    }
}

__device__ __forceinline__ bool bam_consumes_ref(unsigned op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }   // M D N = X

constexpr int BAM_THREADS = 256;   // four wavefronts, one record each at a time

__global__ void __launch_bounds__(BAM_THREADS) k_bam_fields(const uint8_t* bam, const long long* rec_off, long long nrec,
                                                            long long n_ref, const uint8_t* mask, int use_minq, long long minq,
                                                            SamRec* rec, int* keep, long long* name_len,
                                                            unsigned long long* first_bad) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = static_cast<long long>(gridDim.x) * (BAM_THREADS / 64);
    for (long long k = static_cast<long long>(blockIdx.x) * (BAM_THREADS / 64) + (threadIdx.x >> 6); k < nrec; k += nwaves) {
        const long long o = rec_off[k];
        const uint8_t* f = bam + o + 4;
        BamFixed F;                                                  // block_size >= 32 and wholly in the buffer: the locator checked
        const bool fits = bam_layout_ok(bam + o, &F);
        const long long bs = F.bs, l_name = F.l_name, n_cig = F.n_cig, l_seq = F.l_seq;
        const unsigned flag = F.flag;
        const int ref_id = static_cast<int>(rd_u32(f)), pos = static_cast<int>(rd_u32(f + 4));
        const int mapq = f[9];
        const long long fixed = 32 + l_name + 4 * n_cig;
        int kept = 0, bad = 0;
        if (!fits) {
            bad = BAM_LAYOUT;
        } else {
            const bool listed = ref_id >= -1 && ref_id < n_ref;
            kept = !(flag & 4) && (!use_minq || mapq >= minq) && (!mask || (listed && mask[ref_id < 0 ? n_ref : ref_id]));
            if (kept) {
                if (pos == INT_MAX) bad = BAM_POS;
                else if (!listed) bad = BAM_RNAME;
                else if (n_cig == 0) bad = BAM_CIGAR_STAR;
            }
            if (kept && !bad) {
                const uint8_t* cig = f + 32 + l_name;
                long long nops = n_cig;
                const unsigned c0 = rd_u32(cig);
                if (n_cig == 2 && (c0 & 15u) == 4u && (c0 >> 4) == static_cast<unsigned long long>(l_seq) && (rd_u32(cig + 4) & 15u) == 3u) {
                    // the stand-in of a CIGAR above 65 535 ops: lane 0 walks the tags for CG:B,I
                    long long cg_off = -1, cg_n = 0;
                    int tbad = 0;
                    if (lane == 0) {
                        long long p = o + 4 + fixed + (l_seq + 1) / 2 + l_seq;
                        const long long end = o + 4 + bs;
                        while (p < end && !tbad) {               // every turn moves p on by at least 4
                            if (p + 3 > end) { tbad = 1; break; }
                            const bool is_cg = bam[p] == 'C' && bam[p + 1] == 'G';
                            const int ty = bam[p + 2];
                            p += 3;
                            long long sz = bam_type_size(ty);
                            if (ty == 'Z' || ty == 'H') {
                                long long q = p;
                                while (q < end && bam[q]) ++q;
                                sz = q + 1 - p;                  // (beyond the record when there is no NUL)
                            } else if (ty == 'B') {
                                if (p + 5 > end) { tbad = 1; break; }
                                const int sub = bam[p];
                                const long long cnt = rd_u32(bam + p + 1);
                                const int es = bam_type_size(sub);
                                if (!es) { tbad = 1; break; }
                                sz = 5 + cnt * es;
                                if (is_cg && sub == 'I' && cnt >= 1 && cg_off < 0 && p + sz <= end) {
                                    cg_off = p + 5;
                                    cg_n = cnt;
                                } else if (is_cg && (sub != 'I' || cnt < 1)) {
                                    tbad = 1;
                                }
                            } else if (!sz) {
                                tbad = 1;
                            }
                            if (is_cg && ty != 'B') tbad = 1;
                            if (p + sz > end) tbad = 1;
                            p += sz;
                        }
                    }
                    tbad = __shfl(tbad, 0);
                    cg_off = __shfl(cg_off, 0);
                    cg_n = __shfl(cg_n, 0);
                    if (tbad) bad = BAM_TAGS;
                    else if (cg_off >= 0) { cig = bam + cg_off; nops = cg_n; }
                }
                if (!bad) {
                    long long width = 0;
                    bool badop = false, nonclip = false;
                    for (long long i = lane; i < nops; i += 64) {
                        const unsigned v = rd_u32(cig + 4 * i), op = v & 15u;
                        if (op > 8u) badop = true;
                        if (bam_consumes_ref(op)) width += v >> 4;
                        if (op != 4u && op != 5u) nonclip = true;
                    }
                    for (int d = 32; d > 0; d >>= 1) width += __shfl_xor(width, d);
                    if (__ballot(badop)) bad = BAM_CIGAR_OP;
                    else {
                        // .get_clip_length: a leading (trailing) H, then an S once that H is removed
                        const unsigned a0 = rd_u32(cig), z0 = rd_u32(cig + 4 * (nops - 1));
                        const unsigned a1 = nops >= 2 ? rd_u32(cig + 4) : 15u, z1 = nops >= 2 ? rd_u32(cig + 4 * (nops - 2)) : 15u;
                        long long lc = 0, rc = 0;
                        if ((a0 & 15u) == 5u) lc = (a0 >> 4) + ((a1 & 15u) == 4u ? a1 >> 4 : 0u);
                        else if ((a0 & 15u) == 4u) lc = a0 >> 4;
                        if ((z0 & 15u) == 5u) rc = (z0 >> 4) + ((z1 & 15u) == 4u ? z1 >> 4 : 0u);
                        else if ((z0 & 15u) == 4u) rc = z0 >> 4;
                        const long long start = static_cast<long long>(pos) + 1, end = start + width - 1;
                        if (width > INT_MAX || lc > INT_MAX || rc > INT_MAX) bad = BAM_CIGAR_RANGE;
                        else if (!__ballot(nonclip)) bad = BAM_CIGAR_CLIPS;
                        else if (end > INT_MAX || end < -INT_MAX) bad = BAM_END;
                        else if (lane == 0) {
                            SamRec R;
                            R.name_pos = o + 36;
                            R.ref = ref_id < 0 ? static_cast<int>(n_ref) : ref_id;
                            R.start = static_cast<int>(start);
                            R.width = static_cast<int>(width);
                            R.lclip = static_cast<int>(lc);
                            R.rclip = static_cast<int>(rc);
                            R.strand = (flag & 16) ? 1 : 0;
                            rec[k] = R;
                        }
                    }
                }
            }
        }
        if (bad) kept = 0;
        if (lane == 0) {
            keep[k] = kept;
            name_len[k] = kept ? l_name - 1 : 0;
            if (bad) atomicMin(first_bad, (static_cast<unsigned long long>(k) << 4) | static_cast<unsigned>(bad));
        }
    }
}

int bam_hops(const uint8_t* bam, long long nbytes, long long ntiles, unsigned* table, hipStream_t s) {
    hipLaunchKernelGGL(k_bam_hops, dim3(static_cast<unsigned>(ntiles)), dim3(BAM_HOP_THREADS), 0, s, bam, nbytes, table);
    SL_HIP(hipGetLastError());
    return 0;
}

int bam_chain(const unsigned* table, long long nbytes, long long ntiles, long long* entry, hipStream_t s) {
    hipLaunchKernelGGL(k_bam_chain, dim3(1), dim3(64), 0, s, table, nbytes, ntiles, entry);
    SL_HIP(hipGetLastError());
    return 0;
}

int bam_starts_count(const uint8_t* bam, long long nbytes, long long ntiles, const long long* entry, long long* count,
                     long long* term, hipStream_t s) {
    hipLaunchKernelGGL(k_bam_starts<false>, dim3(nblk(ntiles, 64)), dim3(64), 0, s, bam, nbytes, ntiles, entry, count,
                       static_cast<const long long*>(nullptr), static_cast<long long*>(nullptr), term);
    SL_HIP(hipGetLastError());
    return 0;
}

int bam_starts_write(const uint8_t* bam, long long nbytes, long long ntiles, const long long* entry, const long long* base,
                     long long* rec_off, hipStream_t s) {
    hipLaunchKernelGGL(k_bam_starts<true>, dim3(nblk(ntiles, 64)), dim3(64), 0, s, bam, nbytes, ntiles, entry,
                       static_cast<long long*>(nullptr), base, rec_off, static_cast<long long*>(nullptr));
    SL_HIP(hipGetLastError());
    return 0;
}

int bam_fields(const uint8_t* bam, const long long* rec_off, long long nrec, long long n_ref, const uint8_t* mask, int use_minq,
               long long minq, SamRec* rec, int* keep, long long* name_len, unsigned long long* first_bad, hipStream_t s) {
    // one wavefront per record, up to 256 workgroups per CU
    const unsigned grid = static_cast<unsigned>(std::min<long long>(nblk(nrec, BAM_THREADS / 64), static_cast<long long>(ctx().num_cu) * 256));
    hipLaunchKernelGGL(k_bam_fields, dim3(grid), dim3(BAM_THREADS), 0, s, bam, rec_off, nrec, n_ref, mask, use_minq, minq, rec,
                       keep, name_len, first_bad);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
