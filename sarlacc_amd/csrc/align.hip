// align.hip -- quality-weighted read-vs-reference affine-gap DP on gfx950.
//
// Replaces the CPU loop of the reference's reference_align class
// (/root/reference/src/reference_align.cpp:54-181 fill, :231-351 backtrack +
// interval lookup, :353-389 strings) and its three .Call wrappers
// (src/adaptor_align.cpp, src/barcode_align.cpp, src/general_align.cpp).
//
// Mapping (see DESIGN.md "DP kernel"):
//   * one wavefront = up to NGMAX alignments side by side; inside one alignment a
//     lane owns K consecutive reference (adaptor) columns, lanes are skewed by one
//     read row (anti-diagonal wavefront);
//   * per-column state (vertical jump score, previous score of the column) lives in
//     VGPRs; per-row state (score of the column to the left, horizontal jump score,
//     "left cell was a horizontal gap" flag) travels to the next lane with DPP moves
//     (row_shr:1 for 16-lane groups, whose leaders get their column-0 inputs from the
//     DPP fill operand; wave_shr:1 otherwise) -- no LDS on the recurrence path;
//   * read bases + qualities are staged 64 rows at a time into an LDS ring, the
//     5 x navail fp64 cost tables sit in LDS;
//   * traceback needs 4 bits per cell (move + "jump continued" flags; the jump lengths
//     the reference stores are rebuilt during the walk).  adaptor_align (MODE 3) does not
//     produce them in the fill at all: it snapshots the lane state every SNAP_P steps and
//     afterwards recomputes, with codes, only the window above each alignment's landing
//     row (tracked online; it replaces the walk up the last column), which the group's
//     leader lane then walks.  MODE 1/2 stream the codes of every cell with nontemporal
//     stores to a per-wave tile in HBM (general_align's strings; gapopen < 0).
//
// All arithmetic is fp64 add/sub/compare in the reference's order, compiled with
// -ffp-contract=off, so scores are bit-identical to the CPU path.
#include "align_host.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <utility>

namespace sarlacc {

constexpr int NGMAX = 4;   // alignments processed side by side in one wavefront (groups of 16 lanes or more)
constexpr int NGMAX2 = 8;  // ... with two 8-lane alignments interleaved in every 16-lane DPP row (ROWF 2)
constexpr int NGMAX4 = 16; // ... with four 4-lane alignments interleaved in every DPP row (ROWF 4: the framed locator at eight columns per lane)
constexpr int NWAVES = 4;  // wavefronts per workgroup: they share one copy of the cost table in LDS
constexpr int RING = 128;        // staged read positions per alignment (2 x 64)
constexpr int RING_MIRROR = 8;   // the first entries again behind the ring: a block of up to 8 steps reads base + 2u without wrapping
constexpr int RING_SLOT = 256;   // uint16 entries reserved per alignment (512 B: a ring address is base | offset)
constexpr int MAX_REF = 1024;

struct AlignArgs {
    const uint8_t* seq;       // ASCII bases, or 2-bit packed bases when nmask != nullptr
    const uint8_t* nmask;     // packed input only: 1 bit per base, set where the base is not A/C/G/T
    const uint8_t* qual;
    const int64_t* off;
    long long n;
    int R, W, ngroups, local;
    int qoffset, navail;
    double GO, GE;
    const double* tables;     // cost table rows of navail doubles, laid out by build_cost_rows
    int tab_doubles;          // size of `tables`
    int row_bytes;            // navail * sizeof(double)
    const double* rowzero;    // [R+1] scores of DP row 0
    const uint32_t* colbase;  // [R+1] byte offset (inside `tables`) of the rows a column reads
    const uint8_t* refchars;  // [R]
    double* scores;
    int32_t* starts;
    int32_t* ends;
    const int32_t* sec_s;
    const int32_t* sec_e;
    int nsec;
    int32_t* sec_so;
    int32_t* sec_wo;
    void* dirs;
    unsigned long long dirs_per_wave;  // elements per wavefront
    int snap_head, snap_win;           // MODE 3: see SNAP_P
    int* badqual;                      // min index of a read holding a quality below the offset
    int read_base;                     // index of this launch's first read in the caller's batch (chunked host calls)
    long long sec_stride;              // reads per section row of sec_so / sec_wo (the caller's whole batch)
    uint8_t* aln_ref;                  // MODE 2: reversed gapped strings, stride L+R per read
    uint8_t* aln_qry;
    int32_t* aln_len;
    int32_t* edits;
    int wide_maxlen;                   // k_align_wide: the longest read of the launch (sizes of its code tiles and boundary arrays)
    double* wide_bnd;                  // k_align_wide with several strips: per workgroup [2][3][wide_maxlen + 2] row states at a strip's last column
    int wide_band;                     // k_align_wide_q with traceback: codes only for the steps that can hold cells within this many rows of the
                                       // main diagonal (0: codes of every cell); a walk that leaves them puts its read on the redo list
    int* wide_redo;                    // [0] number of reads on the list, [1 ...] their indices (written by the banded launch)
    const int* wide_list;              // the redo launch: the reads to align (count read from the device: wide_list[-1]); null: reads 0 .. n - 1
    // MODE 4 (integer locator fill + fp64 window, see LOC_NEG) and its redo launch
    const int* loc_tab;                // integer cost table: the rows of `tables` scaled by 2^k and rounded, int32 (addressed by colbase / 2)
    const int* loc_rz;                 // [R+1] integer row 0
    int loc_GO, loc_GE, loc_D;         // penalties in integer units (framed: loc_GO is the opening GO - GE); candidate margin D
    int loc_framed;                    // the locator runs in the extension-free frame (MODE 6 instead of MODE 5)
    int loc_force;                     // testing: every read goes on the redo list
    double loc_unit, loc_slack, loc_top;  // 2^-k; Delta_int + eps_fp; sum+ smax + max(0, row 0) + 1 (window certificate)
    int* loc_redo;                     // [0] reads on the redo list, [2 ...] their indices (reset per launch)
    int* loc_stats;                    // summed over a call: [0] reads redone, [1] walks that stalled at the window top, [2] reads the locator
                                       // put on its oversize list, [3] walks that left the LDS code ring, [4 .. 5] one 64-bit count of
                                       // window steps, [6 .. 7] one of the code words such walks read from the global tile (see LOC_STATS)
    int* loc_out;                      // [3 n] per read: I_max, lo, hi (x2 units) from MODE 5 for MODE 4
    // window classes (null: off, MODE 4 takes the reads in index order and lists the oversize ones itself)
    uint8_t* loc_cls;                  // [n] per read: ceil(window steps / 8), 0 for a read on the oversize list
    int* loc_ccount;                   // [LOC_NCLS] reads per class, then [LOC_NCLS] the cursors of k_loc_order (reset per launch)
    int* loc_over;                     // the locator's oversize list, laid out like loc_redo (reset per launch)
    const int* read_list;              // the reads of this launch ([0] count, reads from [2]): a redo list for MODE 3, the window order for
                                       // MODE 4; null: reads 0 .. n - 1
    int bad_done;                      // the locator of this call has seen every quality: this launch reports no bad one (its
                                       // slots are not read indices where it runs from a list)
    int win_nb;                        // MODE 4 with the codes in LDS (WLDS): blocks of the per-wave code ring (see WIN_LDS_WAVES)
};

// Traceback code of one cell, 4 bits -- the raw outcomes of the cell's four comparisons:
//   bit 0  H > V            (horizontal beats vertical)
//   bit 1  M > max(H, V)    (diagonal move; otherwise bit 0 picks horizontal / vertical)
//   bit 2  the horizontal jump was continued here (left_jump_point kept)
//   bit 3  the vertical jump was continued here (up_jump_point kept)
// The reference stores jump LENGTHS (src/reference_align.cpp:139,154,170-177); they are
// recovered during the walk: a horizontal step at column c is 1 + (number of consecutive
// columns c, c-1, ... whose bit 2 is set), a vertical step at row i is 1 + (number of
// consecutive rows i, i-1, ... whose bit 3 is set) -- exactly 1 + pos - left_jump_point and
// 1 + i - up_jump_point.  A lane packs the codes of STEPS consecutive steps x K columns
// into one word, first cell in the top nibble: 0.5 B per cell instead of the 2-4 B of a
// stored length.
// Lane masks (one bit per lane) live in SGPR pairs.  The selects and the traceback-bit packing
// below take them as scalar operands, so all flag logic (and / andn2 / nor) runs on the scalar
// unit and the vector unit sees exactly one instruction per select and one per packed bit.
using mask_t = unsigned long long;
typedef const double __attribute__((address_space(3))) lds_cdouble;
typedef const uint16_t __attribute__((address_space(3))) lds_cu16;
typedef const int __attribute__((address_space(3))) lds_cint;

__device__ __forceinline__ int sel32(int if0, int if1, mask_t m) {
    int r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(if0), "v"(if1), "s"(m));
    return r;
}
// pk = 2 * pk + bit: shifts the word left and drops the lane's mask bit in at the bottom
__device__ __forceinline__ uint32_t push_bit(uint32_t pk, mask_t m) {
    uint32_t r;
    mask_t carry_out;
    asm("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(r), "=s"(carry_out) : "v"(pk), "s"(m));
    return r;
}
__device__ __forceinline__ int hi32(double v) { return static_cast<int>(__double_as_longlong(v) >> 32); }
__device__ __forceinline__ int lo32(double v) { return static_cast<int>(__double_as_longlong(v)); }
__device__ __forceinline__ double mk64(int hi, int lo) {
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// Hand a value to the lane that owns the next columns of the same alignment.  ROWF 1: alignments are 16 lanes wide
// and start on DPP row boundaries (row_shr:1); the first lane of every row -- the leader of an alignment -- has no
// source lane and keeps `keep` (its DP column 0 value: pass the destination itself and the constant set before the
// loop stays there for free).  ROWF 2: two 8-lane alignments share a DPP row, one in the even and one in the odd
// lanes, and the hand-over is row_shr:2 -- lanes 0 and 1 of the row are the two leaders and again have no source.
// Twice the columns per lane at the same width in columns: half the cross-lane moves per cell.  ROWF 4: four 4-lane
// alignments share a DPP row, alignment a in the lanes = a mod 4, the hand-over is row_shr:4 and lanes 0 to 3 of the row
// are the four leaders.  ROWF 0: across
// the whole wave (wave_shr:1), leaders overwrite what arrives.
template <int ROWF>
__device__ __forceinline__ int lane_shr1(int v, int keep) {
    if (ROWF == 1) return __builtin_amdgcn_update_dpp(keep, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    if (ROWF == 2) return __builtin_amdgcn_update_dpp(keep, v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
    if (ROWF == 4) return __builtin_amdgcn_update_dpp(keep, v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
// max(lane_shr1(v, -inf), other): the hand-over of a value whose only consumer is one max.  The fill value is the identity
// of max, so the compiler folds the move into the max itself (v_max_i32 with the DPP modifier, `other` in the destination);
// a leader, which has no source lane, ends with `other`.
template <int ROWF>
__device__ __forceinline__ int lane_shr1_max(int v, int other) {
    static_assert(ROWF == 1 || ROWF == 2 || ROWF == 4, "row shifts only");
    constexpr int NEG = -0x7fffffff - 1;
    if (ROWF == 1) return max(__builtin_amdgcn_update_dpp(NEG, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false), other);
    if (ROWF == 4) return max(__builtin_amdgcn_update_dpp(NEG, v, 0x114 /* row_shr:4 */, 0xf, 0xf, false), other);
    return max(__builtin_amdgcn_update_dpp(NEG, v, 0x112 /* row_shr:2 */, 0xf, 0xf, false), other);
}
template <int ROWF>
__device__ __forceinline__ double lane_shr1(double v, double keep) {
    return mk64(lane_shr1<ROWF>(hi32(v), hi32(keep)), lane_shr1<ROWF>(lo32(v), lo32(keep)));
}

template <int K>
struct TbSteps { static constexpr int value = (8 / K) > 0 ? 8 / K : 1; };
template <int K>
struct TbStore { using type = uint32_t; };
template <>
struct TbStore<16> { using type = unsigned long long; };

template <bool B>
struct Flag { static constexpr bool value = B; };

// MODE 3 (adaptor_align, local, gapopen >= 0): no traceback stream at all.  The fill keeps only
// scores, the landing row of column R and, every SNAP_P steps, a snapshot of the complete lane
// state (column scores, jump scores, the row state in flight between lanes).  Afterwards each
// alignment restores the snapshot just above its landing row and recomputes a window of at
// most SNAP_WIN steps with traceback codes; the leader walks the window and, should the path
// leave it through the top, the next window up is recomputed.  A snapshot is the exact state
// of the recurrence, so the recomputed cells are the cells of the first pass, bit for bit.
constexpr int SNAP_P = 64;      // steps between snapshots (multiple of the 64-row staging block)
// rows above the row a walk asks for that its window must cover: an alignment of R columns
// rarely spans more than R + R/4 rows, and a longer one only costs another window
static inline int snap_head(int R) { return R + R / 4 + 4; }
// steps per window: SNAP_P - 1 + head + W lanes + 1, rounded up to the 8-step store granule
static inline int snap_win(int R, int W) { return (SNAP_P + snap_head(R) + W + 7) / 8 * 8; }

// MODE 4 (adaptor_align, local, gapopen >= 0, dyadic penalties, eight alignments per wave): the same outputs as MODE 3
// without an fp64 fill.  F is the reference's fp64 DP, T the same DP in real arithmetic, GO = gapopen + gapext, GE = gapext.
//   * Pass 1, the locator: the DP in int32 with every cost table entry, row 0, GO and GE scaled by 2^k and the table
//     entries rounded to the nearest integer (-inf -> LOC_NEG).  GO 2^k and GE 2^k must be integers, so the recurrence
//     itself is exact and every path's value is within (R + 1) / 2 units of 2^k times its real value: |I / 2^k - T| <=
//     Delta_int = (R + 1) 2^-(k+1) cell for cell.  fl(a + t) is monotone in a and max is exact, so every cell of F is the
//     fp64 chain of the path it picked and at least the chain of any other path into it; chains whose values are cells
//     stay inside [-(GO + GE R), sum+ smax] and take at most 2R + 4 + (2 sum+ + GO + GE R) / GE rounded operations, which
//     bounds |F - T| by eps_fp (host: plan_locate).  The score is max_i X(i), X(i) = max(match, horizontal) at (i, R), and
//     its landing row l is the first row that reaches it; every row with X(i) = score has I(i) >= I_max - D,
//     D = ceil(2 (Delta_int + eps_fp) 2^k) + 1.  The fill reports I_max and a superset [lo, hi] of those rows, at the
//     granularity of an 8-cell block (lo: the last block that lifted column R by more than D; hi: the last block whose X
//     came within D of column R).
//   * Window certificate.  A path that visits a row above r0 = lo - Wc and reaches (i >= lo, R) other than by a vertical
//     step in column R takes at least Wc + 1 - R vertical steps in columns < R: its real value is at most
//     U = sum+ smax + max(0, row 0) - GO - GE (Wc - R).  Wc is chosen per read from I_max so that U + GO + 1 stays below
//     F_low = I_max 2^-k - Delta_int - eps_fp <= F(l, R) (the + GO covers an alternative that beats a gap continuation of
//     the path, which pays GO instead of GE to rejoin it; the + 1 every rounding of such a chain, checked on the host).
//   * Pass 2: the fp64 DP with traceback codes from r0 (rounded down to 8 rows; r0 < 8: the true row 0) with -inf above it
//     and zeros in column 0, through hi.  Its cells are <= F and >= every path that stays below r0, so every value on the
//     reference's path and every comparison the walk reads (one side on the path, the other only smaller in the window,
//     or, where the other side wins, an alternative the certificate excludes) is the same as in the full DP: the score,
//     the move bits, both "jump continued" bits and the landing row (the last row of the window's column R that improved
//     on the row above).  The walk reads only such cells; one that reaches a row above r0 contradicts the proof and is
//     counted as a stall.
//   * Safety net: a read whose window exceeds the code tile (snap_win steps: two near-equal hits far apart, a weak best
//     hit) or whose walk stalls goes on a device-side list, which the MODE 3 kernel then aligns (read_list).
// Pass 1 runs as a kernel of its own (MODE 5: int32 state only, no walk, a third of the LDS) and hands {I_max, lo, hi} per
// read to the window kernel (MODE 4) through HBM (12 B per read).
// MODE 6 is MODE 5 in the frame I'(i, c) = I(i, c) + GE (i + c) (row 0, column 0 and the jump scores shifted alike), where
// both gap extensions cost 0, an opening costs GO - GE (in column R of local mode every vertical step "costs" -GE) and the
// diagonal move gains 2 GE, folded into the table by the host.  The map is a bijection per cell, so every comparison
// between candidates of one cell comes out as in MODE 5 and the two modes compute the same cells.  Column R's tests
// compare values of different rows of one block: the difference of their frames is a constant folded into D.  The
// frame grows by GE 2^k per row, so the host picks k from the longest read as well (plan_locate) and falls back to MODE 5
// where no k >= LOC_FRAME_KMIN fits.
// ROWF 4: MODE 6 for 25 to 32 columns runs in a shape of its own, eight columns per lane, four lanes per alignment, sixteen
// alignments per wavefront (four interleaved per DPP row, hand-over by row_shr:4), blocks still two rows tall: the work a lane
// does per block beside its cells is shared by sixteen cells instead of eight.  The same cells, and column R's [lo, hi] as the
// eight-lane shape reports them, to the row (see LOC_ODD in k_align); the window kernel keeps its shape, the hand-over is per read.
constexpr int LOC_NEG = -(1 << 29);   // -inf of the integer DP (and of its table entries); cells stay above -2^27
// -inf of a framed table entry.  Framed cells and intermediates lie in (-2^27, 2^30] (plan_locate), so diag' + LOC_NEG_FRAMED
// neither leaves int32 nor passes a real cell: cell (i, c) is at least the horizontal path from column 0,
// H' >= -GO - GE (c - 1) - (R + 1) / 2 + GE (i + c), and diag' <= bpos + (R + 1) / 2 + GE (i + c - 2), so
// diag' + LOC_NEG_FRAMED < H' follows from bpos + GO + GE (c - 3) + (R + 1) < 2^30, which the range rule guarantees (all in
// units of 2^-k).
constexpr int LOC_NEG_FRAMED = -(1 << 30);
constexpr int LOC_FRAME_KMIN = 8;
// resident wavefronts per SIMD of the locator kernel: at 4 it takes 114 VGPRs (115 in the frame) and spills nothing (at 6
// and 8 its steady state reloads spilled registers from scratch).  At eight columns per lane (ROWF 4) it takes all 128 and
// keeps about thirty dwords in scratch, touched at the refills and around the item loop, never inside a steady block
constexpr int LOC_WAVES = 4;
constexpr int LOC_STATS = 8;   // ints of AlignArgs::loc_stats
// The codes of a MODE 4 window in LDS (WLDS).  A walk reads one code word per cell it visits, each load depending on the one
// before, and from the global tile every one of them is an L2 round trip behind an L1 invalidate.  The window's last
// win_nb blocks of code words therefore also stay in a per-wave LDS ring (block b in slot b % win_nb), which holds the
// rows a walk from the window's last row normally visits (snap_head + W steps); a walk that climbs past them reads the
// global tile, the backing store, after the fence the tile needs.  With the ring a workgroup takes about 48 KB of LDS at
// 30 columns, three fit a CU, and the kernel is compiled for three wavefronts per SIMD.
constexpr int WIN_LDS_WAVES = 3;
static inline int win_ring_blocks(int R, int W, int unr) { return (snap_head(R) + W + unr - 1) / unr + 1; }
// Window classes.  A window wave runs the steps of the tallest of its eight windows, so the locator, which ends with
// every input of a read's window plan, files the read under ceil(steps / 8) and k_loc_order turns the class bytes into
// the order MODE 4 takes its reads in: tallest class first, a class contiguous, any order inside it (outputs go by read
// index).  Reads whose window exceeds the code tile go on a list of their own instead, which the snapshot kernel aligns
// on a second stream beside the windows.
constexpr int LOC_NCLS = 32;   // classes 1 .. LOC_NCLS - 1 (snap_win / 8 is 15 at most for the shapes the locator serves)

// The window plan of one read from what the locator reports (lo, hi in x2 units): the window's first row (0: the true
// row 0), the lowest row it must hold and its steps.  The locator and MODE 4 both call this and nothing else.
struct WinPlan { int ts, want, need; };
__device__ __forceinline__ WinPlan window_plan(const AlignArgs& A, int imax, int lo_x2, int hi_x2) {
    const int lo = (lo_x2 >> 1) + 1, hi = (hi_x2 >> 1) + 1;
    // the window certificate: U + GO + 1 < F_low, U = top - 1 - GO - GE (Wc - R)
    const double f_low = static_cast<double>(imax) * A.loc_unit - A.loc_slack;
    const double over = floor((A.loc_top - f_low) / A.GE) + 1.0;
    const int wc = A.R + (over > 0.0 ? static_cast<int>(fmin(over, 1.0e6)) : 0);
    const int r0 = lo - wc;
    const int ts = r0 < 8 ? 0 : (r0 & ~7);
    return {ts, hi, hi + A.W + 1 - ts};
}

// The window order from the class bytes: perm[0] the number of reads in it, perm[2 ...] the reads, tallest class first.
// A block ranks its 256 reads per class in LDS and reserves one range per class with one atomic on the class cursor.
__global__ void __launch_bounds__(256) k_loc_order(const uint8_t* cls, long long n, int* ctl, int* perm) {
    __shared__ int s_cnt[LOC_NCLS], s_base[LOC_NCLS];
    const int t = threadIdx.x;
    if (t < LOC_NCLS) s_cnt[t] = 0;
    __syncthreads();
    const long long read = static_cast<long long>(blockIdx.x) * 256 + t;
    const int c = read < n ? min(static_cast<int>(cls[read]), LOC_NCLS - 1) : 0;
    int rank = 0;
    if (c) rank = atomicAdd(&s_cnt[c], 1);
    __syncthreads();
    if (t < LOC_NCLS) {
        int taller = 0;
        for (int x = t + 1; x < LOC_NCLS; ++x) taller += ctl[x];
        const int mine = t ? s_cnt[t] : 0;
        s_base[t] = taller + (mine ? atomicAdd(&ctl[LOC_NCLS + t], mine) : 0);
        if (blockIdx.x == 0 && t == 0) perm[0] = taller;   // every class is taller than class 0, which holds no read
    }
    __syncthreads();
    if (c) perm[2 + s_base[c] + rank] = static_cast<int>(read);
}

// MODE 0: scores only.  MODE 1: scores + reference->read map (adaptor_align), codes streamed.
// MODE 2: scores + gapped strings + edit distance (general_align).
// MODE 3: as MODE 1 by snapshots + windowed recompute (LOCAL, !PENSEL only; see SNAP_P).
// MODE 4: as MODE 3 by an integer locator fill + one fp64 window (ROWF 2 only; see LOC_NEG).
// MODE 5 / 6: the locator fill of MODE 4 as a kernel of its own, plain / in the extension-free frame.
// LOCAL: free leading read bases + free vertical gaps in the last column (adaptor mode).
// ROWF: 0 alignments of any width, wave-wide shifts; 1 alignments are 16 lanes wide and start on DPP row
// boundaries; 2 alignments are 8 lanes wide, two interleaved per DPP row (see lane_shr1); 4 alignments are 4 lanes wide,
// four interleaved per DPP row (the framed locator at K = 8 only).
// KLAST: index (inside its lane) of reference column R when known at compile time, else -1.
// PENSEL: select the gap penalty of every step explicitly (only needed when gapopen < 0).
//
// Penalty selection.  The reference charges a gap step "extension" instead of "open +
// extension" when the cell it leaves was itself reached by a gap of the same kind
// (src/reference_align.cpp:125-158).  In that case the cell's score IS the running jump
// score (best == H == lj, bit for bit), so the reference's candidate `left - GE` equals the
// jump continuation `lj - GE` exactly, the comparison `continuation > candidate` is false and
// the maximum is the continuation.  With gapopen >= 0 the candidate `left - GO` is <= that
// continuation, so max(continuation, left - GO) is the same double: the kernel always
// subtracts the opening penalty and selects nothing.  Only the "jump continued" flag differs
// (true instead of false), and the true flag is raw && !(previous cell's move is the same gap
// kind) -- the traceback applies that from the neighbour's code, which it reads anyway.
template <int K, int MODE, bool LOCAL, int ROWF, int KLAST, bool PENSEL, bool WLDS = false, int LTRIM = 0>
// (six wavefronts per SIMD for the snapshot mode; five with eight alignments per wavefront: four columns per lane need the registers --
// at six the recompute code spilled -- 2 182 -> 2 213 GCUPS on the same box)
// (WLDS: the MODE 4 window with its codes in an LDS ring and the walk by whole lane groups, three wavefronts per SIMD, see WIN_LDS_WAVES)
__global__ void __launch_bounds__(64 * NWAVES, WLDS ? WIN_LDS_WAVES : MODE >= 5 ? LOC_WAVES : (MODE == 3 && ROWF != 2) ? 6 : 5) k_align(const AlignArgs A) {
    constexpr bool ROW16 = ROWF != 0;                      // leaders keep their column-0 inputs through the DPP fill operand
    constexpr int NG = ROWF == 4 ? NGMAX4 : ROWF == 2 ? NGMAX2 : NGMAX;   // alignments per wavefront at most
    // uint16 entries per alignment's ring slot: 512 B slots let a ring address be base | offset; with eight
    // alignments per wave the slots are packed (ring + mirror) and the address is an add
    constexpr int SLOT = (ROWF == 2 || ROWF == 4) ? RING + RING_MIRROR : RING_SLOT;
    // (ROWF 4 is the locator alone, which writes no codes: its blocks stay two rows tall, the granularity of [lo, hi])
    constexpr int UNR = ROWF == 4 ? 2 : TbSteps<K>::value;
    constexpr int CELLS = UNR * K;
    using Word = typename TbStore<K>::type;
    constexpr bool ADDC = sizeof(Word) == 4;
    // LDS: read rings first (256 B per alignment, so a ring address is base | offset), then the
    // cost table shared by the waves of the workgroup, then the per-wave reference->read maps
    extern __shared__ __align__(256) unsigned char smem[];
    static_assert(RING * sizeof(uint16_t) == 256 && RING + RING_MIRROR <= RING_SLOT, "ring addressing assumes 256 B of ring inside a 512 B slot");
    constexpr int RING_BYTES = NWAVES * NG * SLOT * static_cast<int>(sizeof(uint16_t));
    static_assert(RING_BYTES % 8 == 0 && (SLOT * sizeof(uint16_t)) % 8 == 0, "table and 8-byte ring stores stay aligned");
    double* const s_tab = reinterpret_cast<double*>(smem + RING_BYTES);
    // LDS byte address of smem (256-aligned), for hand-built LDS addresses
    const int lds0 = static_cast<int>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)smem));

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // tell the compiler it is wave-uniform
    // ROWF 4: the locator's own shape, four lanes per alignment and sixteen alignments, whatever the window kernel's (A.W,
    // A.ngroups: window_plan sizes the windows by them)
    const int W = ROWF == 4 ? 4 : A.W, R = A.R, NGR = ROWF == 4 ? NGMAX4 : A.ngroups;
    // lane <-> (alignment g of the wave, lane j inside it)
    auto lane_of = [&](int gg, int jj) -> int {
        return ROWF == 4 ? ((gg >> 2) << 4) + (jj << 2) + (gg & 3) : ROWF == 2 ? ((gg >> 1) << 4) + (jj << 1) + (gg & 1) : gg * W + jj;
    };
    const int g = ROWF == 4 ? (((lane >> 4) << 2) | (lane & 3)) : ROWF == 2 ? (((lane >> 4) << 1) | (lane & 1)) : lane / W;
    const int j = ROWF == 4 ? ((lane & 15) >> 2) : ROWF == 2 ? ((lane & 15) >> 1) : lane - g * W;
    const bool lane_on = g < NGR;
    const bool leader = (j == 0);
    const int c0 = j * K + 1;
    const double NEG_INF = -__builtin_huge_val();
    const double GO = A.GO, GE = A.GE;
    const int GOhi = hi32(GO), GOlo = lo32(GO), GEhi = hi32(GE), GElo = lo32(GE);

    static_assert(MODE < 4 || ((ROWF == 2 || ROWF == 4) && LOCAL && !PENSEL), "the locator runs the interleaved local shapes only");
    static_assert(ROWF != 4 || (MODE == 6 && K == 8 && KLAST >= 0), "four alignments per DPP row: the framed locator at eight columns per lane");
    static_assert(!WLDS || MODE == 4, "the LDS code ring belongs to the MODE 4 window");
    // the redo launch after a locator pass with an empty list: nothing to stage
    if (A.read_list && A.read_list[0] == 0) return;
    // MODE 5 / 6: the integer table (4-byte entries, rows half as long) in place of the fp64 one
    constexpr bool LOCATOR = MODE >= 5, FRAMED = MODE == 6;
    int* const s_tabi = reinterpret_cast<int*>(smem + RING_BYTES);
    if (LOCATOR)
        for (int x = threadIdx.x; x < A.tab_doubles; x += 64 * NWAVES) s_tabi[x] = A.loc_tab[x];
    else
        for (int x = threadIdx.x; x < A.tab_doubles; x += 64 * NWAVES) s_tab[x] = A.tables[x];
    uint16_t* const s_ring = reinterpret_cast<uint16_t*>(smem) + wave * NG * SLOT;
    int32_t* const s_map = reinterpret_cast<int32_t*>(s_tab + A.tab_doubles) + wave * A.ngroups * (R + 1);
    // WLDS: the wave's code ring behind the maps, win_nb blocks of 64 words; this lane's word of slot 0
    const int code_ring_bytes = WLDS ? A.win_nb * 64 * static_cast<int>(sizeof(Word)) : 0;
    unsigned char* const s_code = reinterpret_cast<unsigned char*>(reinterpret_cast<int32_t*>(s_tab + A.tab_doubles) + NWAVES * A.ngroups * (R + 1)) +
                                  wave * code_ring_bytes;
    int code_ofs = 0;              // byte offset of the ring slot the next block's codes go to (wave-uniform)
    int walk_glob = 0, walks_out = 0;   // WLDS: code words this lane read from the global tile; leaders: walks that read any

    double vgo[K], vge[K], rz[K];
    int colbase[K];  // LDS byte address of the table rows this column reads (see build_tables)
    int colbi[K], vgoi[K], vgei[K], rzi[K];   // MODE 4: the same for the integer DP
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = c0 + k;
        // columns past R (last lane when K does not divide R) reuse column R's tables: they
        // compute garbage that nothing reads (their outputs only feed a leader or an idle lane)
        const int cc = c <= R ? c : R;
        colbase[k] = lds0 + RING_BYTES + static_cast<int>(A.colbase[cc]);
        // only column R is "last"; with KLAST known it sits at k == KLAST, every other k takes the penalties from SGPRs
        const bool last = LOCAL && cc == R && (KLAST < 0 || k == KLAST);
        vgo[k] = last ? 0.0 : GO;
        vge[k] = last ? 0.0 : GE;
        rz[k] = A.rowzero[cc];
        if (LOCATOR) {
            colbi[k] = lds0 + RING_BYTES + static_cast<int>(A.colbase[cc] >> 1);
            // framed: loc_GO is the opening GO - GE and an extension is free; the free vertical step of column R gains GE.
            // Column R's jump score is the running maximum of the rows above, never more than the cell just above, so its
            // "extension" may cost anything that keeps it there: 0, the constant of the other columns
            vgoi[k] = last ? (FRAMED ? -A.loc_GE : 0) : A.loc_GO;
            vgei[k] = FRAMED ? 0 : last ? 0 : A.loc_GE;
            rzi[k] = A.loc_rz[cc];
        }
    }
    const double rz_left = A.rowzero[c0 - 1 <= R ? c0 - 1 : R];
    const int jlast = (R - 1) / K, klast = KLAST >= 0 ? KLAST : (R - 1) % K;
    const long long gwave = static_cast<long long>(blockIdx.x) * NWAVES + wave;
    const long long nwaves = static_cast<long long>(gridDim.x) * NWAVES;
    Word* const scr = static_cast<Word*>(A.dirs) + static_cast<size_t>(gwave) * A.dirs_per_wave;
    // MODE 3: the tile holds the codes of one window, the snapshots follow it
    constexpr int NSV = 2 * K + 3;  // doubles per lane in a snapshot
    double* const snap = reinterpret_cast<double*>(scr + static_cast<size_t>(A.snap_win / UNR) * 64);
    const int ring_g = lds0 + (wave * NG + g) * static_cast<int>(SLOT * sizeof(uint16_t));  // byte address of this alignment's ring
    __syncthreads();

    const long long nreads = A.read_list ? static_cast<long long>(A.read_list[0]) : A.n;   // redo launch: the list's length
    const long long nitems = (nreads + NGR - 1) / NGR;
    int wsteps = 0;   // MODE 4: window steps of this wave's items (wave-uniform; a wave owns a few items of 120 steps at most)
    for (long long item = gwave; item < nitems; item += nwaves) {
        const long long slot_r = item * NGR + g;
        const bool valid = lane_on && slot_r < nreads;
        const long long read = A.read_list ? (valid ? static_cast<long long>(A.read_list[2 + slot_r]) : 0) : slot_r;
        long long start = 0;
        int L = 0;
        if (valid) {
            start = A.off[read];
            L = static_cast<int>(A.off[read + 1] - start);
        }
        // wave-uniform description of the (up to NG) reads of this work item, kept in SGPRs
        long long gstart[NG];
        int glen[NG];
        int Lmax = 0, Lmin = 0x7fffffff;
        int Lmin8[2] = {0x7fffffff, 0x7fffffff};   // ROWF 4: of the item's first and second eight reads (an item each in the eight-lane shape)
#pragma unroll
        for (int gg = 0; gg < NG; ++gg) {
            const int src = gg < NGR ? lane_of(gg, 0) : 0;
            const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(start), src));
            const int hi = __builtin_amdgcn_readlane(static_cast<int>(start >> 32), src);
            const int len = __builtin_amdgcn_readlane(L, src);
            gstart[gg] = (static_cast<long long>(hi) << 32) | lo;
            glen[gg] = gg < NGR ? len : 0;
            Lmax = max(Lmax, glen[gg]);
            // reads past the end of the batch (last work item) compute garbage nobody stores
            if (gg < NGR && item * NGR + gg < nreads) {
                Lmin = min(Lmin, glen[gg]);
                if (ROWF == 4) Lmin8[gg >> 3] = min(Lmin8[gg >> 3], glen[gg]);
            }
        }

        // Read staging, one refill (64 positions per alignment) ahead of use: lane -> (alignment sg = lane / 16, four
        // consecutive positions), so one pass of the wave stages four alignments (two passes for eight, four for sixteen).  A staged entry
        // is the byte offset of (base code, quality) inside a block of table rows; base codes 0-3 = ACGT, 4 = anything else.
        constexpr int NPASS = NG / 4;
        const int sq = (lane & 15) * 4;
        int sgs[NPASS], slens[NPASS], stoffs[NPASS];   // per pass: the alignment this lane stages, its length, its window start (toff[sg])
        long long sstarts[NPASS];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            sgs[ps] = (lane >> 4) + 4 * ps;
            const int sgl = sgs[ps] < NGR ? lane_of(sgs[ps], 0) : 0;
            const int slen_any = __shfl(L, sgl);   // every lane takes part: a source lane switched off would read as 0
            slens[ps] = sgs[ps] < NGR ? slen_any : 0;
            sstarts[ps] = (static_cast<long long>(__shfl(static_cast<int>(start >> 32), sgl)) << 32) |
                          static_cast<unsigned>(__shfl(static_cast<int>(start), sgl));
            stoffs[ps] = 0;
        }
        // four qualities (one per byte); four 2-bit base codes | four exception bits << 8.  RAWPF (the locator with LTRIM & 2):
        // what the loads returned and nothing else, so that no wait for them stands between a refill and the next one, where
        // stage4 decodes them -- q the four quality bytes and, ASCII reads, b the four characters, both taken from the read's
        // last four bytes where fewer than four positions are left (stage4 shifts); packed reads, b / b2 and m / m2 the
        // bytes of the bases and of the mask that hold the first and the last of the positions
        struct Pf { uint32_t q, b, b2, m, m2; };
        constexpr bool RAWPF = MODE == 6 && (LTRIM & 2) != 0;
        auto fetch4 = [&](int slen, long long sstart, int r0) -> Pf {
            const int r = r0 + sq;
            const int nv = min(max(slen - r, 0), 4);
            Pf v{0u, 0u, 0u, 0u, 0u};
            if (nv == 0) return v;
            const long long idx = sstart + r;
            if (RAWPF) {   // every byte read lies inside the read, or is a byte of packed bases / mask that holds one of its positions
                if (slen >= 4) {
                    const long long at = idx - (4 - nv);
                    __builtin_memcpy(&v.q, A.qual + at, 4);
                    if (!A.nmask) __builtin_memcpy(&v.b, A.seq + at, 4);
                } else {   // a read of one to three bases
                    for (int e = 0; e < nv; ++e) {
                        v.q |= static_cast<uint32_t>(A.qual[idx + e]) << (8 * e);
                        if (!A.nmask) v.b |= static_cast<uint32_t>(A.seq[idx + e]) << (8 * e);
                    }
                }
                if (A.nmask) {
                    const long long last = idx + nv - 1;
                    v.b = A.seq[idx >> 2];
                    v.b2 = A.seq[last >> 2];
                    v.m = A.nmask[idx >> 3];
                    v.m2 = A.nmask[last >> 3];
                }
                return v;
            }
            if (nv == 4) {
                __builtin_memcpy(&v.q, A.qual + idx, 4);   // every byte read lies inside the read (no over-read of caller memory)
                if (A.nmask) {  // 2-bit packed bases + exception mask (sarlacc_dev_pack_reads)
                    const uint32_t two = (A.seq[idx >> 2] | (static_cast<uint32_t>(A.seq[(idx + 3) >> 2]) << 8)) >> ((idx & 3) * 2);
                    const uint32_t exc = (A.nmask[idx >> 3] | (static_cast<uint32_t>(A.nmask[(idx + 3) >> 3]) << 8)) >> (idx & 7);
                    v.b = (two & 0xffu) | ((exc & 0xfu) << 8);
                } else {
                    uint32_t s4;
                    __builtin_memcpy(&s4, A.seq + idx, 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t b = (s4 >> (8 * e)) & 0xffu;
                        const uint32_t x = (b >> 1) & 3u, code = x ^ (x >> 1);         // A C G T -> 0 1 2 3
                        const uint32_t exc = ((0x54474341u >> (8 * code)) & 0xffu) != b;   // anything else
                        v.b |= (code << (2 * e)) | (exc << (8 + e));
                    }
                }
                return v;
            }
            for (int e = 0; e < nv; ++e) {   // the last positions of a read
                v.q |= static_cast<uint32_t>(A.qual[idx + e]) << (8 * e);
                uint32_t code, exc;
                if (A.nmask) {
                    code = (A.seq[(idx + e) >> 2] >> (((idx + e) & 3) * 2)) & 3u;
                    exc = (A.nmask[(idx + e) >> 3] >> ((idx + e) & 7)) & 1u;
                } else {
                    const uint32_t b = A.seq[idx + e];
                    code = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 0u;
                    exc = !(b == 'A' || b == 'C' || b == 'G' || b == 'T');
                }
                v.b |= (code << (2 * e)) | (exc << (8 + e));
            }
            return v;
        };
        auto stage4 = [&](int sg, int slen, int r0, Pf v, long long sstart = 0) {
            const int r = r0 + sq;
            uint32_t ent[4];
            bool bad = false;
            if (RAWPF) {   // into the decoded form; what lies past the read's last position is masked below
                const int nv = min(max(slen - r, 0), 4);
                const int back = (slen >= 4 && nv > 0) ? 8 * (4 - nv) : 0;
                v.q >>= back;
                if (A.nmask) {
                    const long long idx = sstart + r;
                    const uint32_t two = (v.b | (v.b2 << 8)) >> ((idx & 3) * 2), exc = (v.m | (v.m2 << 8)) >> (idx & 7);
                    v.b = (two & 0xffu) | ((exc & 0xfu) << 8);
                } else {
                    const uint32_t s4 = v.b >> back;
                    v.b = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t b = (s4 >> (8 * e)) & 0xffu;
                        const uint32_t x = (b >> 1) & 3u, code = x ^ (x >> 1);         // A C G T -> 0 1 2 3
                        const uint32_t exc = ((0x54474341u >> (8 * code)) & 0xffu) != b;   // anything else
                        v.b |= (code << (2 * e)) | (exc << (8 + e));
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int qi = static_cast<int>(static_cast<signed char>((v.q >> (8 * e)) & 0xffu)) - A.qoffset;
                bad = bad || (r + e < slen && qi < 0);
                qi = qi < 0 ? 0 : (qi >= A.navail ? A.navail - 1 : qi);
                const uint32_t code = ((v.b >> (8 + e)) & 1u) ? 4u : ((v.b >> (2 * e)) & 3u);
                // the locator's ring is its own: it stages offsets into the int32 rows, half of an fp64 row offset
                const uint32_t at = LOCATOR ? code * static_cast<uint32_t>(A.row_bytes >> 1) + static_cast<uint32_t>(qi << 2)
                                            : code * static_cast<uint32_t>(A.row_bytes) + static_cast<uint32_t>(qi << 3);
                ent[e] = (r + e < slen) ? at : 0u;
            }
            if (bad && !A.bad_done) atomicMin(A.badqual, A.read_base + static_cast<int>(item * NGR + sg));
            const uint2 w = make_uint2(ent[0] | (ent[1] << 16), ent[2] | (ent[3] << 16));
            uint16_t* const slot = s_ring + sg * SLOT + (r & (RING - 1));   // r is a multiple of 4: 8-byte aligned
            *reinterpret_cast<uint2*>(slot) = w;
            if ((r & (RING - 1)) < RING_MIRROR) *reinterpret_cast<uint2*>(slot + RING) = w;
        };
        Pf pf[NPASS];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) pf[ps] = fetch4(slens[ps], sstarts[ps], 0);
        int toff[NG];  // first step of the window being recomputed (MODE 3), per alignment; 0 in the fill
#pragma unroll
        for (int gg = 0; gg < NG; ++gg) toff[gg] = 0;

        // per-column state: score of the previous row, vertical jump score (and, PENSEL only,
        // the penalty the next vertical step pays)
        double S[K], UJ[K];
        int vp_hi[K], vp_lo[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { S[k] = rz[k]; UJ[k] = NEG_INF; vp_hi[k] = hi32(vgo[k]); vp_lo[k] = lo32(vgo[k]); }
        // per-row state arriving from the lane to the left: score, horizontal jump score (PENSEL:
        // and the penalty a horizontal step from that cell pays).  Leaders keep column-0 constants.
        double s_in = 0.0, lj_in = NEG_INF, diag_prev = rz_left;
        int ph_in = GOhi, pl_in = GOlo;
        // Row position as x2 = 2 * (i - 1), i = t - j: doubles as the ring byte offset.
        int x2 = -2 * j - 2;
        int x2max = valid ? 2 * L - 2 : -2;
        // Landing row of the upward walk the traceback performs in column R (tracked by the lane
        // owning that column, in x2 units): land[i] = i if the move at (i,R) is not vertical, else
        // the landing row of the cell the vertical jump leads to.  Without it the walk up the last
        // column (free vertical gaps => ~L single steps in local mode) costs ~L dependent loads.
        int land_prev = -2, land_up = -2;
        int vnl = 0;  // the move at (i-1, R) was a vertical gap
        // MODE 3 tracks the landing row directly: in local mode the vertical gaps of column R are
        // free, every row of a vertical run resets the jump (its candidate S[i-1] equals the
        // running jump score, and the comparison is strict), so the walk up column R stops at the
        // last row whose move is not vertical, i.e. the last row with best > V.
        int land_x2 = -2;

        // Steps [t_begin, t_end).  GUARD = false is the steady state: every lane of every
        // alignment of the wave is inside its read, nothing is predicated and all flags are
        // lane masks in SGPRs.
        // TR: 0 no traceback, 1 codes streamed to the per-wave tile (MODE 1/2), 2 landing row +
        // snapshots (MODE 3 fill), 3 codes of a recomputed window (MODE 3; t counts from toff[]), 5 codes + landing row of
        // the MODE 4 window
        auto run = [&](auto guard_tag, auto trace_tag, int t_begin, int t_end) {
            constexpr bool GUARD = decltype(guard_tag)::value;
            constexpr int TR = decltype(trace_tag)::value;
            constexpr bool CODES = TR == 1 || TR == 3 || TR == 5;
            constexpr bool LAND = TR == 2 || TR == 5;
            mask_t m_vnl = GUARD ? 0 : __builtin_amdgcn_ballot_w64(vnl != 0);
            for (int t0 = t_begin; t0 < t_end; t0 += UNR) {
                if ((t0 & 63) == 0) {
                    int t0s = t0;   // opaque copy: keeps the staging addresses out of the step loop's induction variables
                    asm volatile("" : "+s"(t0s));
#pragma unroll
                    for (int ps = 0; ps < NPASS; ++ps) {
                        stage4(sgs[ps], slens[ps], stoffs[ps] + t0s, pf[ps]);
                        pf[ps] = fetch4(slens[ps], sstarts[ps], stoffs[ps] + t0s + 64);
                    }
                    if (TR == 2 && (t0 & (SNAP_P - 1)) == 0) {
                        // complete lane state before step t0
                        double* sp = snap + static_cast<size_t>(t0 / SNAP_P) * (NSV * 64) + lane;
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            __builtin_nontemporal_store(S[k], sp + (2 * k) * 64);
                            __builtin_nontemporal_store(UJ[k], sp + (2 * k + 1) * 64);
                        }
                        __builtin_nontemporal_store(s_in, sp + (2 * K) * 64);
                        __builtin_nontemporal_store(lj_in, sp + (2 * K + 1) * 64);
                        __builtin_nontemporal_store(diag_prev, sp + (2 * K + 2) * 64);
                    }
                }
                Word pk = 0;
                double v_first = 0.0;   // TR 2: vertical candidate of column R at the block's first step
                // ring address of the block's first row; the following rows sit behind it (mirror: no wrap inside a block)
                const uint32_t ring_blk = static_cast<uint32_t>(ROWF == 2 || ROWF == 4 ? ring_g + (x2 & 0xff) : (ring_g | (x2 & 0xff)));
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    if (ROWF == 0) {
                        // column 0 of the DP (src/reference_align.cpp:63-78): what a leader lane consumes
                        const int im1 = x2 >> 1;
                        const double col0 = (LOCAL || im1 < 0) ? 0.0 : (-GO - GE * static_cast<double>(im1));
                        if (leader) { s_in = col0; lj_in = NEG_INF; ph_in = GOhi; pl_in = GOlo; }
                    }
                    double left = s_in, lj = lj_in;
                    int ph = ph_in, pl = pl_in;
                    const double s_two_back = diag_prev;  // what s_in held two steps ago
                    bool act = true;
                    if (GUARD) act = x2 >= 0 && x2 <= x2max;
                    if (act) {
                        const int rd = *reinterpret_cast<lds_cu16*>(ring_blk + 2u * u);
                        double diag = diag_prev;
                        diag_prev = s_in;
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            // Every "if (a > b) {x = a} else {a = b}" pair of the reference leaves
                            // max(a, b) in both; no NaN or -0 can occur on this path, so fmax is the
                            // same value bit for bit (src/reference_align.cpp:125-158).
                            const double hcand = left - (PENSEL ? mk64(ph, pl) : GO);
                            const double ljm = lj - GE;
                            const bool b_hj = ljm > hcand;
                            const double H = fmax(ljm, hcand);
                            lj = H;
                            const double vcand = S[k] - (PENSEL ? mk64(vp_hi[k], vp_lo[k]) : vgo[k]);
                            const double ujm = UJ[k] - vge[k];
                            const bool b_vj = ujm > vcand;
                            const double V = fmax(ujm, vcand);
                            UJ[k] = V;
                            const double w = *reinterpret_cast<lds_cdouble*>(static_cast<uint32_t>(colbase[k] + rd));
                            const double M = diag + w;
                            diag = S[k];
                            // (:164-174): M only if greater than both, else H only if greater than V
                            const bool b_hv = H > V;
                            const double G = fmax(H, V);
                            const bool b_tm = M > G;
                            const double best = fmax(M, G);
                            S[k] = best;
                            left = best;
                            const bool is_last = KLAST >= 0 ? (k == KLAST) : (k == klast);
                            if (!GUARD) {
                                const mask_t m_hj = __builtin_amdgcn_ballot_w64(b_hj), m_vj = __builtin_amdgcn_ballot_w64(b_vj);
                                const mask_t m_hv = __builtin_amdgcn_ballot_w64(b_hv), m_tm = __builtin_amdgcn_ballot_w64(b_tm);
                                const mask_t m_vn = ~(m_hv | m_tm);  // the move here is a vertical gap
                                if (PENSEL) {
                                    const mask_t m_hp = m_hv & ~m_tm;  // the move here is a horizontal gap
                                    ph = sel32(GOhi, GEhi, m_hp);
                                    pl = sel32(GOlo, GElo, m_hp);
                                    vp_hi[k] = sel32(hi32(vgo[k]), hi32(vge[k]), m_vn);
                                    vp_lo[k] = sel32(lo32(vgo[k]), lo32(vge[k]), m_vn);
                                }
                                if (LAND && is_last) {
                                    // Column R's score never decreases down the rows (free vertical gaps), so
                                    // "some row of this block improved it" is one comparison per block: the
                                    // score after the block against the running maximum before it.  The
                                    // block's last row is recorded; the walk steps up the <= UNR - 1 vertical
                                    // moves to the exact landing row through the recomputed codes.
                                    if (u == 0) v_first = V;
                                    if (u == UNR - 1) land_x2 = sel32(land_x2, x2, __builtin_amdgcn_ballot_w64(best > v_first));
                                }
                                if (CODES) {
                                    if (ADDC) {
                                        pk = push_bit(push_bit(push_bit(push_bit(static_cast<uint32_t>(pk), m_vj), m_hj), m_tm), m_hv);
                                    } else {
                                        const unsigned raw = (b_hv ? 1u : 0u) | (b_tm ? 2u : 0u) | (b_hj ? 4u : 0u) | (b_vj ? 8u : 0u);
                                        pk |= static_cast<Word>(raw) << (4 * (CELLS - 1 - (u * K + k)));
                                    }
                                    if (TR == 1 && is_last) {
                                        const mask_t m_cont = m_vj & ~m_vnl;  // the vertical jump really continued
                                        land_up = sel32(land_prev, land_up, m_cont);  // continued: same landing row
                                        land_prev = sel32(land_up, x2, ~m_vn);
                                        m_vnl = m_vn;
                                    }
                                }
                            } else {
                                const bool hp = b_hv && !b_tm, vn = !b_hv && !b_tm;
                                if (PENSEL) {
                                    ph = hp ? GEhi : GOhi;
                                    pl = hp ? GElo : GOlo;
                                    vp_hi[k] = vn ? hi32(vge[k]) : hi32(vgo[k]);
                                    vp_lo[k] = vn ? lo32(vge[k]) : lo32(vgo[k]);
                                }
                                if (LAND) {
                                    if (is_last && best > V) land_x2 = x2;
                                }
                                if (CODES) {
                                    const unsigned raw = (b_hv ? 1u : 0u) | (b_tm ? 2u : 0u) | (b_hj ? 4u : 0u) | (b_vj ? 8u : 0u);
                                    pk |= static_cast<Word>(raw) << (4 * (CELLS - 1 - (u * K + k)));
                                    if (TR == 1 && is_last) {
                                        const bool cont = b_vj && vnl == 0;
                                        land_up = cont ? land_up : land_prev;
                                        land_prev = vn ? land_up : x2;
                                        vnl = vn ? 1 : 0;
                                    }
                                }
                            }
                        }
                    }
                    // hand the row state to the next lane; with 16-lane groups the leaders have no
                    // source lane and keep their column-0 values
                    if (ROW16 && !LOCAL) {
                        const int i = (x2 >> 1) + 1;  // global mode: column 0 changes with the row
                        const double col0_next = (i < 0) ? 0.0 : (-GO - GE * static_cast<double>(i));
                        s_in = lane_shr1<ROWF>(left, col0_next);
                    } else if (ROW16 && !GUARD) {
                        // s_in itself stays live as the next step's diagonal; the register that
                        // held it two steps ago is free and, on leader lanes, holds the same 0.0
                        s_in = lane_shr1<ROWF>(left, s_two_back);
                    } else {
                        s_in = lane_shr1<ROWF>(left, s_in);
                    }
                    lj_in = lane_shr1<ROWF>(lj, lj_in);
                    if (PENSEL) {
                        ph_in = lane_shr1<ROWF>(ph, ph_in);
                        pl_in = lane_shr1<ROWF>(pl, pl_in);
                    }
                    x2 += 2;
                }
                if (TR == 1) __builtin_nontemporal_store(pk, scr + static_cast<size_t>(t0 / UNR) * 64 + lane);
                if (TR == 3 || TR == 5) scr[static_cast<size_t>(t0 / UNR) * 64 + lane] = pk;
                if (TR == 5 && WLDS) {
                    *reinterpret_cast<Word*>(s_code + code_ofs + lane * static_cast<int>(sizeof(Word))) = pk;
                    code_ofs += 64 * static_cast<int>(sizeof(Word));
                    if (code_ofs == code_ring_bytes) code_ofs = 0;
                }
            }
            if (!GUARD) vnl = sel32(0, 1, m_vnl);
        };

        const int nsteps = ((Lmax + W + UNR - 1) / UNR) * UNR;
        int t_a = ((W + UNR - 1) / UNR) * UNR;                 // every lane has entered its read
        int t_b = Lmin == 0x7fffffff ? 0 : ((Lmin + 1) / UNR) * UNR;  // first block leaving the shortest read
        t_a = min(t_a, nsteps);
        t_b = min(max(t_b, t_a), nsteps);
        // (The framed locator's ROWF 4 shape restates these three for the ROWF 2 shape at K = 4 -- t_a = 8, t_b even and from the
        // shortest of eight reads, two-row blocks -- to report the same [lo, hi]: see LOC_SHIFT below and change both together.
        // Where they part, results stay right and only class bytes and the oversize list differ;
        // tests/test_gpu_align_locate_k8.py compares the records of the two shapes read for read.)
        // MODE 5, pass 1 (see LOC_NEG): the lane of column R ends with I_max and the candidate rows [lo, hi] (x2 units),
        // which MODE 4 reads back
        int loc_max = 0, loc_lo = -2, loc_hi = -2;
        if constexpr (MODE == 4) {
            if (valid && j == jlast) {
                loc_max = A.loc_out[3 * read];
                loc_lo = A.loc_out[3 * read + 1];
                loc_hi = A.loc_out[3 * read + 2];
            }
        } else if constexpr (LOCATOR) {
            // Sg: Si less the column's vertical opening, carried beside it across blocks (Si itself is the next diagonal)
            int Si[K], Sg[K], UJi[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { Si[k] = rzi[k]; Sg[k] = rzi[k] - vgoi[k]; UJi[k] = LOC_NEG; }
            int si_in = 0, lji_in = LOC_NEG, di_prev = A.loc_rz[c0 - 1 <= R ? c0 - 1 : R];
            const int GOi = A.loc_GO, GEi = A.loc_GE, D = A.loc_D;
            // framed: a block's last row lies UNR - 1 rows, that many GE, above its first in the frame
            const int D_lo = FRAMED ? D + (UNR - 1) * GEi : D;
            // LTRIM & 1 (framed steady state): the horizontal jump score stays in the lane that formed it and its hand-over
            // rides on the consumer's max (see lane_shr1_max); lj_src is that score before the move
            constexpr bool FOLD = FRAMED && (LTRIM & 1) != 0;
            // ROWF 4 with 25 to 28 columns (KLAST < 4): the steady state's blocks start on odd steps, see below
            constexpr bool LOC_ODD = ROWF == 4 && KLAST < 4;
            constexpr int LOC_SHIFT = LOC_ODD ? 3 : 4;
            // ROWF 4 reports what the eight-lane shape reports, to the row.  [lo, hi] are exact rows in the guarded phases and
            // block rows in the steady state, so column R must take the same rows by the same rule in the same blocks.  In
            // that shape its lane, (R - 1) / 4, is 6 or 7 and its steady state covers the steps 8 to t_b of the read's own
            // eight reads; here its lane is 3, LOC_SHIFT steps earlier on every row -- on odd steps where that lane was 6.  The
            // steady state ends with the shorter of the item's two halves; the rows the other half would still have run in its
            // steady state (steps below blk_end) take the block rule in the guarded phase.
            int ta = t_a, tb = t_b, tn = nsteps, blk_end = 0;
            if (ROWF == 4) {
                // the partner: {K = 4, W = 8, ngroups = 8, rowf = 2} with two-row blocks (plan_align picks ROWF 4 beside no other)
                static_assert(TbSteps<4>::value == 2 && NGMAX4 == 2 * NGMAX2, "ROWF 4 mirrors the schedule of the eight-lane shape at K = 4");
                auto tb8 = [](int lmin) { return max(lmin == 0x7fffffff ? 0 : ((lmin + 1) / 2) * 2, 8); };   // (t_a = 8 <= nsteps there)
                tn = Lmax + 4;
                ta = min(8 - LOC_SHIFT, tn);
                tb = min(max(tb8(Lmin) - LOC_SHIFT, ta), tn);
                blk_end = tb8(g < 8 ? Lmin8[0] : Lmin8[1]) - LOC_SHIFT;
            }
            auto run_loc = [&](auto guard_tag, int t_begin, int t_end) {
                constexpr bool GUARD = decltype(guard_tag)::value;
                constexpr int NO_ROW = -0x7fffffff - 1;
                int hi_blk = NO_ROW;   // steady state: first row of the last block that sets loc_hi (the row loc_lo takes too)
                int g_before = 0, g_xacc = LOC_NEG;   // ROWF 4, guarded: s_before and xacc of a block taken row by row
                int lj_src = 0;
                // what row_shr:2 (ROWF 4: row_shr:4) will bring back: lji_in of the lane two (four) to the right (the leaders'
                // LOC_NEG is implied)
                if (FOLD && !GUARD)
                    lj_src = ROWF == 4 ? __builtin_amdgcn_update_dpp(lji_in, lji_in, 0x104 /* row_shl:4 */, 0xf, 0xf, false)
                                       : __builtin_amdgcn_update_dpp(lji_in, lji_in, 0x102 /* row_shl:2 */, 0xf, 0xf, false);
                // RAWPF: nothing the item's first loads returned is still in flight when the steady state begins, so its blocks
                // hold no wait for global memory (the refills' own loads are waited for at the next refill)
                if (RAWPF && !GUARD) __builtin_amdgcn_s_waitcnt(0x0f70 /* vmcnt(0) */);
                for (int t0 = t_begin; t0 < t_end; t0 += UNR) {
                    // (blocks on odd steps, see LOC_ODD, refill one step early: the ring holds 128 positions, a lane reads
                    // at most four behind the wave's first)
                    const int t0r = LOC_ODD ? t0 + (t0 & 1) : t0;
                    if ((t0r & 63) == 0) {
                        int t0s = t0r;
                        asm volatile("" : "+s"(t0s));
#pragma unroll
                        for (int ps = 0; ps < NPASS; ++ps) {
                            stage4(sgs[ps], slens[ps], t0s, pf[ps], sstarts[ps]);
                            pf[ps] = fetch4(slens[ps], sstarts[ps], t0s + 64);
                        }
                    }
                    int s_before = 0, xacc = LOC_NEG;   // column R before the block; max of X over the block
                    const uint32_t ring_blk = static_cast<uint32_t>(ring_g + (x2 & 0xff));
                    // staged entries are byte offsets into the int32 rows; the steady state reads a block's entries up front
                    int rdv[UNR];
                    if (!GUARD) {
#pragma unroll
                        for (int u = 0; u < UNR; ++u) rdv[u] = static_cast<int>(*reinterpret_cast<lds_cu16*>(ring_blk + 2u * u));
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        if (GUARD && ROWF == 4 && t0 + u >= t_end) break;   // (its phases end on any step)
                        int left = si_in, lj = lji_in;
                        const int s_two_back = di_prev;
                        bool act = true;
                        if (GUARD) act = x2 >= 0 && x2 <= x2max;
                        if (act) {
                            const int rd = GUARD ? static_cast<int>(*reinterpret_cast<lds_cu16*>(ring_blk + 2u * u)) : rdv[u];
                            int diag = di_prev;
                            di_prev = si_in;
                            int lg = si_in - GOi;   // the cell to the left less the opening
#pragma unroll
                            for (int k = 0; k < K; ++k) {
                                const int H = (FOLD && !GUARD && k == 0) ? lane_shr1_max<ROWF>(lj_src, lg) : max(FRAMED ? lj : lj - GEi, lg);
                                lj = H;
                                const int V = max(UJi[k] - vgei[k], Sg[k]);
                                UJi[k] = V;
                                const int M = diag + *reinterpret_cast<lds_cint*>(static_cast<uint32_t>(colbi[k] + rd));
                                diag = Si[k];
                                const int X = max(M, H);
                                const int best = max(X, V);
                                Si[k] = best;
                                left = best;
                                // one subtraction serves the next column of this row and this column of the next row
                                lg = best - GOi;
                                Sg[k] = (KLAST >= 0 && k != KLAST) ? lg : best - vgoi[k];
                                const bool is_last = KLAST >= 0 ? (k == KLAST) : (k == klast);
                                if (is_last) {
                                    // V is column R's running maximum before this row (free vertical gaps)
                                    if (GUARD && ROWF == 4 && t0 + u >= ta && t0 + u < blk_end) {
                                        if (((t0 + u - ta) & 1) == 0) {
                                            g_before = V;
                                            g_xacc = X;
                                        } else {
                                            g_xacc = max(g_xacc, X - GEi);
                                            const int bd = best - D_lo;
                                            if (bd > g_before) loc_lo = x2 - 2;
                                            if (g_xacc >= bd) loc_hi = x2;
                                        }
                                    } else if (GUARD) {
                                        if (best - D > V) loc_lo = x2;
                                        if (X + D >= best) loc_hi = x2;
                                    } else {
                                        if (u == 0) s_before = V;
                                        xacc = u == 0 ? X : max(xacc, FRAMED ? X - u * GEi : X);   // in the frame of the block's first row
                                        if (u == UNR - 1) {
                                            const int bd = best - D_lo, xb = x2 - 2 * (UNR - 1);
                                            loc_lo = sel32(loc_lo, xb, __builtin_amdgcn_ballot_w64(bd > s_before));
                                            hi_blk = sel32(hi_blk, xb, __builtin_amdgcn_ballot_w64(xacc >= bd));
                                        }
                                    }
                                }
                            }
                        }
                        // framed: column 0, which the leaders keep, is GE i; the register of two steps back holds GE (i - 1)
                        if (FRAMED) si_in = GUARD ? lane_shr1<ROWF>(left, GEi * ((x2 >> 1) + 2)) : lane_shr1<ROWF>(left, s_two_back + 2 * GEi);
                        else si_in = GUARD ? lane_shr1<ROWF>(left, si_in) : lane_shr1<ROWF>(left, s_two_back);
                        if (FOLD && !GUARD) lj_src = lj;
                        else lji_in = lane_shr1<ROWF>(lj, lji_in);
                        x2 += 2;
                    }
                }
                if (FOLD && !GUARD) lji_in = lane_shr1<ROWF>(lj_src, lji_in);   // the leaders keep their LOC_NEG
                if (!GUARD && hi_blk != NO_ROW) loc_hi = hi_blk + 2 * (UNR - 1);
            };
            run_loc(Flag<true>{}, 0, ta);
            run_loc(Flag<false>{}, ta, tb);
            run_loc(Flag<true>{}, tb, tn);
            loc_max = Si[0];
#pragma unroll
            for (int k = 1; k < K; ++k) loc_max = (k == klast) ? Si[k] : loc_max;
            if (FRAMED) loc_max -= GEi * (L + R);   // out of the frame: column R's last row is the read's last
            if (valid && j == jlast) {
                A.loc_out[3 * read] = loc_max;
                A.loc_out[3 * read + 1] = loc_lo;
                A.loc_out[3 * read + 2] = loc_hi;
                if (A.loc_cls) {
                    const WinPlan wp = window_plan(A, loc_max, loc_lo, loc_hi);
                    int cls = 0;
                    if (wp.need > A.snap_win || A.loc_force) {
                        const int at = atomicAdd(A.loc_over, 1);
                        A.loc_over[2 + at] = static_cast<int>(read);
                        atomicAdd(A.loc_stats, 1);
                        atomicAdd(A.loc_stats + 2, 1);
                    } else {
                        cls = min(max((wp.need + 7) >> 3, 1), LOC_NCLS - 1);
                        atomicAdd(A.loc_ccount + cls, 1);
                    }
                    A.loc_cls[read] = static_cast<uint8_t>(cls);
                }
            }
            continue;
        } else {
            constexpr int TR_FILL = MODE == 3 ? 2 : (MODE >= 1 ? 1 : 0);
            run(Flag<true>{}, Int<TR_FILL>{}, 0, t_a);
            run(Flag<false>{}, Int<TR_FILL>{}, t_a, t_b);
            run(Flag<true>{}, Int<TR_FILL>{}, t_b, nsteps);
        }

        if (MODE < 4 && valid && j == jlast) {
            double sc = S[0];
#pragma unroll
            for (int k = 1; k < K; ++k) sc = (k == klast) ? S[k] : sc;
            A.scores[read] = sc;
        }

        if (MODE == 3 || MODE == 4) {
            int32_t* map = s_map + g * (R + 1);
            const Word* const wtile = scr;
            // walk state of the group's leader: position, and the jump chain being measured (MODE 4: the row is set
            // after the window)
            int row = (__shfl(land_x2, lane_of(g, jlast)) >> 1) + 1, c = R;
            int phase = 0, chain_n = 0, chain_at = 0;
            unsigned cur = 0;
            int want = row;         // lowest row the next window has to hold
            int pending = valid ? 1 : 0;
            // every round moves at least one alignment to an earlier snapshot, so the number of rounds
            // is bounded; the explicit bound guarantees that the wave leaves the loop whatever the codes say
            int rounds_left = MODE == 4 ? 1 : (Lmax + W) / SNAP_P + 8;
            int ts4 = 0;            // MODE 4: first row of the window (0: the true row 0)
            auto push_redo = [&]() {   // MODE 4: the MODE 3 kernel aligns this read
                const int at = atomicAdd(A.loc_redo, 1);
                A.loc_redo[2 + at] = static_cast<int>(read);
                atomicAdd(A.loc_stats, 1);
            };
            if (MODE == 4) {
                const int lane_r = lane_of(g, jlast);
                const WinPlan wp = window_plan(A, __shfl(loc_max, lane_r), __shfl(loc_lo, lane_r), __shfl(loc_hi, lane_r));
                ts4 = wp.ts;
                want = wp.want;
                // (with window classes the locator has listed these reads already and the order holds none of them)
                if (valid && (wp.need > A.snap_win || A.loc_force)) {
                    if (leader) push_redo();
                    pending = 0;
                }
            }
            while (__builtin_amdgcn_ballot_w64(pending != 0)) {
                if (--rounds_left < 0) {
                    if (lane == 0) atomicExch(A.badqual + 1, 1);
                    break;
                }
                // ---- recompute the window that holds row `want` (per alignment) ----
                const int ts = !pending ? 0 : MODE == 4 ? ts4 : (max(want - A.snap_head, 0) / SNAP_P) * SNAP_P;
                // steps [0, nwin) of the window; [t_wa, t_wb) of them have every lane of every
                // pending alignment inside its read (the others compute garbage nobody reads)
                int nwin = 0, t_wa = 0, t_wb = 0x7fffffff;
#pragma unroll
                for (int gg = 0; gg < NG; ++gg) {
                    const int src = gg < NGR ? lane_of(gg, 0) : 0;
                    toff[gg] = __builtin_amdgcn_readlane(ts, src);
                    const int pend = __builtin_amdgcn_readlane(pending, src);
                    const int need = __builtin_amdgcn_readlane(want + W + 1 - ts, src);
                    if (gg < NGR && pend) {
                        nwin = max(nwin, need);
                        if (toff[gg] < W) t_wa = W;                 // lanes still entering the read
                        t_wb = min(t_wb, glen[gg] + 1 - toff[gg]);  // first step leaving it
                    }
                }
                nwin = min(((nwin + UNR - 1) / UNR) * UNR, A.snap_win);
                if (MODE == 4) wsteps += nwin;
                t_wa = min(((t_wa + UNR - 1) / UNR) * UNR, nwin);
                t_wb = min(max((t_wb / UNR) * UNR, t_wa), nwin);
                // (MODE 3 reads snapshots next; the MODE 4 window reads nothing this wave wrote to global memory)
                if (!WLDS) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                }
                code_ofs = 0;
                if (MODE == 3) {
                    const double* sp = snap + static_cast<size_t>(ts / SNAP_P) * (NSV * 64) + lane;
#pragma unroll
                    for (int k = 0; k < K; ++k) { S[k] = sp[(2 * k) * 64]; UJ[k] = sp[(2 * k + 1) * 64]; }
                    s_in = sp[(2 * K) * 64];
                    lj_in = sp[(2 * K + 1) * 64];
                    diag_prev = sp[(2 * K + 2) * 64];
                } else {
                    // ts > 0: -inf above row ts, zeros in column 0 (the leaders' inputs); ts == 0: the true row 0
                    const bool fresh = ts > 0;
#pragma unroll
                    for (int k = 0; k < K; ++k) { S[k] = fresh ? NEG_INF : rz[k]; UJ[k] = NEG_INF; }
                    s_in = (fresh && !leader) ? NEG_INF : 0.0;
                    lj_in = NEG_INF;
                    diag_prev = fresh ? (leader ? 0.0 : NEG_INF) : rz_left;
                    land_x2 = -2;
                }
                x2 = 2 * (ts - j - 1);
                x2max = pending ? 2 * L - 2 : -2;
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    const int q = lane >> 4;   // sgs[ps] = q + 4 * ps
                    stoffs[ps] = q == 0 ? toff[4 * ps] : q == 1 ? toff[4 * ps + 1] : q == 2 ? toff[4 * ps + 2] : toff[4 * ps + 3];
                    // the rows just above the window (lanes 1 .. W - 1 start there); MODE 4 windows may start at any multiple of 8
                    if (stoffs[ps] >= 64) stage4(sgs[ps], slens[ps], stoffs[ps] - 64, fetch4(slens[ps], sstarts[ps], stoffs[ps] - 64));
                    else if (MODE == 4 && stoffs[ps] > 0) stage4(sgs[ps], slens[ps], 0, fetch4(slens[ps], sstarts[ps], 0));
                    pf[ps] = fetch4(slens[ps], sstarts[ps], stoffs[ps]);
                }
                constexpr int TR_WIN = MODE == 4 ? 5 : 3;
                run(Flag<true>{}, Int<TR_WIN>{}, 0, t_wa);
                run(Flag<false>{}, Int<TR_WIN>{}, t_wa, t_wb);
                run(Flag<true>{}, Int<TR_WIN>{}, t_wb, nwin);
                // WLDS: the walk reads the ring its own wave wrote, in LDS order; the tile's fences wait for the first word
                // a walk takes from it (tile_word)
                if (WLDS) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                } else {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                }
                // WLDS: the window's last block and its ring slot; block b <= last_blk sits (last_blk - b) slots before it
                const int last_blk = nwin / UNR - 1;
                const int last_ofs = (code_ofs ? code_ofs : code_ring_bytes) - 64 * static_cast<int>(sizeof(Word));
                bool tile_fenced = false;
                // rows above this one hold no cell of the full DP (MODE 4 with a fresh boundary)
                const int rtop = (MODE == 4 && ts > 0) ? ts : 0;
                if (MODE == 4) {
                    // the score and the landing row come from the window (column R through hi >= l)
                    row = (__shfl(land_x2, lane_of(g, jlast)) >> 1) + 1;
                    if (pending && j == jlast) {
                        double sc = S[0];
#pragma unroll
                        for (int k = 1; k < K; ++k) sc = (k == klast) ? S[k] : sc;
                        A.scores[read] = sc;
                    }
                }

                // ---- leaders walk (src/reference_align.cpp:231-278) until done or out of window ----
                // WLDS: the eight lanes of an alignment walk together.  Every lane carries the leader's state and runs the
                // leader's code, so the group stays in step; in a run of diagonal moves, most of the path, lane m looks at
                // the cell m steps up the diagonal and a ballot gives the length of the run: one LDS round trip for up to
                // eight cells.  Only the leader writes outputs and lists.
                constexpr bool GWALK = WLDS;
                if (pending && (GWALK || leader)) {
                    // the code word of lane `ln` at step tt >= 0 of the window: from the ring while the block is one of its
                    // last win_nb, else from the global tile (`counted`: the read goes into align_walk_global)
                    auto tile_word = [&](int tt, int ln, bool counted) -> Word {
                        const unsigned b = static_cast<unsigned>(tt) / UNR;
                        if (WLDS) {
                            const unsigned back = static_cast<unsigned>(last_blk) - b;
                            if (back < static_cast<unsigned>(A.win_nb)) {
                                int o = last_ofs - static_cast<int>(back) * 64 * static_cast<int>(sizeof(Word));
                                o += o < 0 ? code_ring_bytes : 0;
                                return *reinterpret_cast<const Word*>(s_code + o + ln * static_cast<int>(sizeof(Word)));
                            }
                            if (!tile_fenced) {   // this wave's tile stores, past its L1
                                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                                tile_fenced = true;
                            }
                            walk_glob += counted ? 1 : 0;
                        }
                        return wtile[b * 64u + static_cast<unsigned>(ln)];
                    };
                    // raw compare bits of cell (rr, cc), see nibble() below; false: above the window
                    auto code_at = [&](int cc, int rr, unsigned& out) -> bool {
                        const int jj = (cc - 1) / K, kk = (cc - 1) % K;
                        const int tt = rr + jj - ts;
                        if (tt < 0 || rr < rtop) return false;
                        const Word w = tile_word(tt, lane_of(g, jj), leader);
                        out = static_cast<unsigned>(w >> (4 * (CELLS - 1 - ((tt % UNR) * K + kk)))) & 15u;
                        return true;
                    };
                    bool stalled = false;
                    while (c > 0 && !stalled) {
                        if (phase == 0) {
                            // runs of diagonal moves (most of the path) in a loop of their own
                            while (!GWALK && c > 0 && row > 0) {
                                const int jj = (c - 1) / K, kk = (c - 1) % K;
                                const int tt = row + jj - ts;
                                if (tt < 0 || row < rtop) break;
                                const Word w = tile_word(tt, lane_of(g, jj), true);
                                if (!((w >> (4 * (CELLS - 1 - ((tt % UNR) * K + kk)))) & 2u)) break;
                                map[c] = row * 2 + 1;
                                --row; --c;
                            }
                            while (GWALK && c > 0 && row > 0) {
                                // lane m of the alignment: is cell (row - m, c - m) inside the window and a diagonal move?
                                const int rr = row - j, cc = c - j;
                                bool on = false;
                                if (cc > 0 && rr > 0) {
                                    const int jj = (cc - 1) / K, kk = (cc - 1) % K;
                                    const int tt = rr + jj - ts;
                                    if (tt >= 0 && rr >= rtop) {
                                        const Word w = tile_word(tt, lane_of(g, jj), true);
                                        on = ((w >> (4 * (CELLS - 1 - ((tt % UNR) * K + kk)))) & 2u) != 0;
                                    }
                                }
                                // the alignment's eight lanes (every second lane of its DPP row) are all here; its bits of
                                // the ballot, packed: bit m = lane m's cell ends the run
                                const mask_t off_m = __builtin_amdgcn_ballot_w64(!on);
                                unsigned x = static_cast<unsigned>(off_m >> lane_of(g, 0)) & 0x5555u;
                                x = (x | (x >> 1)) & 0x3333u;
                                x = (x | (x >> 2)) & 0x0f0fu;
                                x = (x | (x >> 4)) & 0xffu;
                                const int len = __builtin_ctz(x | 0x100u);   // diagonal moves from (row, c) on, 8 at most
                                if (j < len) map[cc] = rr * 2 + 1;
                                row -= len; c -= len;
                                if (len < 8) break;
                            }
                            if (c <= 0) break;
                            if (row <= 0) { map[c] = (row + 1) * 2; --c; continue; }  // D[c][0] = 1
                            unsigned nb;
                            if (!code_at(c, row, nb)) { want = row; stalled = true; break; }
                            if (nb & 2u) { map[c] = row * 2 + 1; --row; --c; continue; }
                            cur = nb;
                            chain_n = 0;
                            phase = (nb & 1u) ? 1 : 2;
                            chain_at = (nb & 1u) ? c : row;
                        }
                        if (phase == 1) {  // horizontal jump: count the columns it continued through
                            while ((cur & 4u) && chain_at > 1) {
                                unsigned prev;
                                if (!code_at(chain_at - 1, row, prev)) { want = row; stalled = true; break; }
                                if ((prev & 3u) == 1u) break;
                                ++chain_n; --chain_at; cur = prev;
                            }
                            if (stalled) break;
                            for (int x = 0; x <= chain_n; ++x) { map[c] = (row + 1) * 2; --c; }
                            phase = 0;
                        } else {           // vertical jump: count the rows it continued through
                            while ((cur & 8u) && chain_at > 1) {
                                unsigned prev;
                                if (!code_at(c, chain_at - 1, prev)) { want = chain_at - 1; stalled = true; break; }
                                if ((prev & 3u) == 0u) break;
                                ++chain_n; --chain_at; cur = prev;
                            }
                            if (stalled) break;
                            row -= 1 + chain_n;  // up moves leave the map untouched (:286)
                            phase = 0;
                        }
                    }
                    if (GWALK) {   // a walk any of whose lanes read the tile left the ring
                        const mask_t out_m = __builtin_amdgcn_ballot_w64(tile_fenced);
                        if (leader && ((out_m >> lane_of(g, 0)) & 0x5555u)) ++walks_out;
                    }
                    if (MODE == 4 && stalled) {
                        if (leader) {
                            atomicAdd(A.loc_stats + 1, 1);
                            push_redo();
                        }
                        pending = 0;
                    }
                    if (!stalled) pending = 0;
                    if (!stalled && leader) {
                        // (src/reference_align.cpp:307-351), size_t wrap kept via unsigned
                        auto interval = [&](int a, int b, bool gaps, unsigned& s, unsigned& e) {
                            if (!gaps) {
                                s = map[a + 1] >> 1;
                                e = (map[b] >> 1) + (map[b] & 1);
                            } else {
                                s = (a == 0) ? 1u : static_cast<unsigned>((map[a] >> 1) + (map[a] & 1));
                                e = (b + 1 == R + 1) ? static_cast<unsigned>(L + 1) : static_cast<unsigned>(map[b + 1] >> 1);
                            }
                            s -= 1;
                            e -= 1;
                        };
                        unsigned s, e;
                        interval(0, R, false, s, e);
                        const bool nonempty = s < e;
                        A.starts[read] = nonempty ? static_cast<int32_t>(s + 1) : 0;
                        A.ends[read] = nonempty ? static_cast<int32_t>(e) : 0;
                        for (int x = 0; x < A.nsec; ++x) {
                            interval(A.sec_s[x], A.sec_e[x], true, s, e);
                            A.sec_so[static_cast<long long>(x) * A.sec_stride + read] = static_cast<int32_t>(s + 1);
                            A.sec_wo[static_cast<long long>(x) * A.sec_stride + read] = static_cast<int32_t>(e - s);
                        }
                    }
                }
                pending = __shfl(pending, lane_of(g, 0));
                want = __shfl(want, lane_of(g, 0));
            }
        }

        if (MODE == 1 || MODE == 2) {
            // make this wave's traceback stores visible to its leader lanes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const int land = (__shfl(land_prev, lane_of(g, jlast)) >> 1) + 1;  // where the walk up column R ends
            if (valid && leader) {
                // raw compare bits of cell (row, c): 1 H>V, 2 M>max(H,V), 4 horizontal jump
                // continuation beat the step from the left, 8 same for the vertical jump
                auto nibble = [&](int c, int row) -> unsigned {  // 1 <= c <= R, 1 <= row <= L
                    const int jj = (c - 1) / K, kk = (c - 1) % K;
                    const int tt = row + jj;
                    const Word w = scr[static_cast<size_t>(tt / UNR) * 64 + lane_of(g, jj)];
                    return static_cast<unsigned>(w >> (4 * (CELLS - 1 - ((tt % UNR) * K + kk)))) & 15u;
                };
                // direction value the reference would have stored at (row, c); a jump continues
                // through a cell only if the cell it came from was not itself entered by the
                // same kind of gap (see "Penalty selection" above)
                auto loadD = [&](int c, int row) -> int {
                    if (row <= 0) return 1;  // D[c][0] = 1 (src/reference_align.cpp:118)
                    unsigned nb = nibble(c, row);
                    if (nb & 2u) return 0;
                    int n = 0;
                    if (nb & 1u) {
                        int x = c;
                        while ((nb & 4u) && x > 1) {
                            const unsigned prev = nibble(x - 1, row);
                            if ((prev & 3u) == 1u) break;
                            ++n; --x; nb = prev;
                        }
                        return 1 + n;
                    }
                    int y = row;
                    while ((nb & 8u) && y > 1) {
                        const unsigned prev = nibble(c, y - 1);
                        if ((prev & 3u) == 0u) break;
                        ++n; --y; nb = prev;
                    }
                    return -(1 + n);
                };
                int row = L, c = R;
                if (MODE == 1) {
                    int32_t* map = s_map + g * (R + 1);
                    row = land;  // up moves leave the map untouched (src/reference_align.cpp:286)
                    while (c > 0) {
                        int d = loadD(c, row);
                        while (row > 0 && d < 0) { row += d; d = loadD(c, row); }
                        if (d == 0) { map[c] = row * 2 + 1; --row; --c; }
                        else { for (int x = 0; x < d; ++x) { map[c] = (row + 1) * 2; --c; } }
                    }
                    // (src/reference_align.cpp:307-351), size_t wrap kept via unsigned
                    auto interval = [&](int a, int b, bool gaps, unsigned& s, unsigned& e) {
                        if (!gaps) {
                            s = map[a + 1] >> 1;
                            e = (map[b] >> 1) + (map[b] & 1);
                        } else {
                            s = (a == 0) ? 1u : static_cast<unsigned>((map[a] >> 1) + (map[a] & 1));
                            e = (b + 1 == R + 1) ? static_cast<unsigned>(L + 1) : static_cast<unsigned>(map[b + 1] >> 1);
                        }
                        s -= 1;
                        e -= 1;
                    };
                    unsigned s, e;
                    interval(0, R, false, s, e);
                    const bool nonempty = s < e;
                    A.starts[read] = nonempty ? static_cast<int32_t>(s + 1) : 0;
                    A.ends[read] = nonempty ? static_cast<int32_t>(e) : 0;
                    for (int x = 0; x < A.nsec; ++x) {
                        interval(A.sec_s[x], A.sec_e[x], true, s, e);
                        A.sec_so[static_cast<long long>(x) * A.sec_stride + read] = static_cast<int32_t>(s + 1);
                        A.sec_wo[static_cast<long long>(x) * A.sec_stride + read] = static_cast<int32_t>(e - s);
                    }
                } else {
                    // gapped strings, emitted from the end (src/reference_align.cpp:353-389)
                    const long long base = start + read * static_cast<long long>(R);
                    uint8_t* oref = A.aln_ref + base;
                    uint8_t* oqry = A.aln_qry + base;
                    const uint8_t* sq = A.seq + start;
                    int m = 0, ed = 0;
                    for (; row > land; --row) { oref[m] = '-'; oqry[m] = sq[row - 1]; ++m; ++ed; }
                    while (c > 0) {
                        int d = loadD(c, row);
                        while (row > 0 && d < 0) {
                            for (int x = 0; x < -d; ++x) { oref[m] = '-'; oqry[m] = sq[row - 1]; ++m; ++ed; --row; }
                            d = loadD(c, row);
                        }
                        if (d == 0) {
                            const uint8_t rc = A.refchars[c - 1], qc = sq[row - 1];
                            oref[m] = rc; oqry[m] = qc; ++m;
                            ed += rc != qc;
                            --row; --c;
                        } else {
                            for (int x = 0; x < d; ++x) { oref[m] = A.refchars[c - 1]; oqry[m] = '-'; ++m; ++ed; --c; }
                        }
                    }
                    while (row > 0) { oref[m] = '-'; oqry[m] = sq[row - 1]; ++m; ++ed; --row; }
                    A.aln_len[read] = m;
                    A.edits[read] = ed;
                }
            }
        }
    }
    if (MODE == 4 && lane == 0 && wsteps) atomicAdd(reinterpret_cast<unsigned long long*>(A.loc_stats + 4), static_cast<unsigned long long>(wsteps));
    if (WLDS && walks_out) atomicAdd(A.loc_stats + 3, walks_out);
    if (WLDS && walk_glob) atomicAdd(reinterpret_cast<unsigned long long*>(A.loc_stats + 6), static_cast<unsigned long long>(walk_glob));
}

// Empty reference: the DP has only column 0 (src/reference_align.cpp:63-78,:104).
__global__ void k_align_emptyref(const int64_t* off, long long n, int local, double GO, double GE,
                                 double* scores, int32_t* starts, int32_t* ends, int nsec,
                                 int32_t* sec_so, int32_t* sec_wo, int32_t* aln_len, int32_t* edits,
                                 const uint8_t* seq, uint8_t* aln_ref, uint8_t* aln_qry) {
    const long long r = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (r >= n) return;
    const int L = static_cast<int>(off[r + 1] - off[r]);
    scores[r] = (local || L < 1) ? 0.0 : (-GO - GE * static_cast<double>(L - 1));
    if (starts) { starts[r] = 0; ends[r] = 0; }
    for (int x = 0; x < nsec; ++x) { sec_so[x * n + r] = 1; sec_wo[x * n + r] = 0; }
    if (aln_len) {
        // every read base sits opposite a gap; strings are stored reversed
        for (int m = 0; m < L; ++m) { aln_ref[off[r] + m] = '-'; aln_qry[off[r] + m] = seq[off[r] + L - 1 - m]; }
        aln_len[r] = L;
        edits[r] = L;
    }
}

// ---------------------------------------------------------------------------
// References of more than MAX_REF columns (qualityAlign against a transcript or a genomic
// region, src/general_align.cpp:12-16; src/reference_align.cpp:7-13 takes any length).
// k_align keeps one alignment inside a wavefront (at most 64 lanes x 16 columns); here ONE
// WORKGROUP holds the alignment: thread t owns K consecutive columns, threads are skewed by one
// read row exactly as k_align's lanes are, and the row state (score of the column to the left,
// "that cell was a horizontal gap", running horizontal jump score) goes to the next thread
// through a double-buffered LDS slot, one barrier per step.  The recurrence is the reference's
// statement for statement (explicit penalty selects, strict >, src/reference_align.cpp:108-181),
// fp64, -ffp-contract=off.  Traceback: 4 bits per cell -- move (0 diagonal, 1 horizontal,
// 2 vertical) + "horizontal jump continued here" + "vertical jump continued here" -- one word per
// thread and step, stored by step so that a step's words are contiguous; the jump LENGTHS the
// reference stores (:131,147) are 1 + the run of continued flags that ends in the cell, and the
// walk (thread 0) counts them.  Read positions are staged WIDE_CH rows at a time into an LDS
// ring as (base code * row bytes + quality * 8), the byte offset inside a column's cost rows.
constexpr int WIDE_CH = 512;      // rows staged per refill
constexpr int WIDE_RING = 2048;   // ring entries (> WIDE_CH + 1024 threads)
constexpr int WIDE_MAXT = 1024;

template <int K>
struct WideWord { using type = uint32_t; };

// The walk of one alignment of k_align_wide / k_align_wide_q, run by ONE wavefront (lane = 0 .. 63) after the codes of every
// strip are in `dirs` (word of thread tt at step s: dirs[strip * strip_words + s * Rw + tt], column k of the thread in nibble K - 1 - k).
// k_align_wide_q's band of steps that carry codes, per wavefront w of an alignment of L rows against R columns (K = 8 columns per
// lane): the cells within `band` rows of the main diagonal i = c L / R sit, for the 512 columns of wavefront w, at its steps
// [lo, hi] (lane l is at row sg - l + 1).  The fill switches its codes on one step before lo (the flags a cell's codes take from the
// row above are then in place at lo); the walk may read the codes of a cell iff its step lies in [lo, hi] or in the first 63
// steps of its wavefront, which always carry codes.
struct WideBand {
    int band, L, R;
    __device__ __forceinline__ int lo(int w) const { return static_cast<int>(512ll * w * L / R) - band - 2; }
    __device__ __forceinline__ int hi(int w) const { return static_cast<int>((512ll * (w + 1) * L + R - 1) / R) + band + 64; }
    __device__ __forceinline__ bool stored(int c, int row) const {   // 1 <= c <= R, 1 <= row <= L
        if (band <= 0) return true;
        const int t = (c - 1) >> 3, w = t >> 6, sg = row + (t & 63) - 1;
        return sg < 63 || (sg >= lo(w) && sg <= hi(w));
    }
};

// (`wb`: the band of stored codes, null = every cell; a walk that needs a cell outside it stops and returns false -- nothing it wrote counts)
template <int K, int MODE, bool STRIPS>
__device__ __forceinline__ bool wide_walk(const AlignArgs& A, typename WideWord<K>::type* dirs, long long strip_words, int CS, long long Rw,
                                          int L, int R, long long read, long long start, int lane, const WideBand* wb = nullptr) {
    using Word = typename WideWord<K>::type;
    bool left_band = false;
    auto ok = [&](int c, int row) -> bool { return !wb || wb->stored(c, row); };
    // The walk, on the first wavefront: the path of a global alignment of like sequences is mostly diagonal, so lane m
    // looks at the cell m steps up the diagonal from (row, c), a ballot gives the length of the diagonal run and its
    // moves are written side by side -- one memory round trip per run instead of one per cell; gaps are taken one
    // run at a time (every lane follows, the outputs are spread over the lanes).
    auto nibble = [&](int c, int row) -> unsigned {   // 1 <= c <= R, 1 <= row <= L
        const int sc = STRIPS ? (c - 1) / CS : 0, cc = (c - 1) - sc * CS;   // strip, column inside it
        const int tt = cc / K, kk = cc % K;
        const Word w = dirs[sc * strip_words + static_cast<long long>(row + tt) * Rw + tt];
        return static_cast<unsigned>(w >> (4 * (K - 1 - kk))) & 15u;
    };
    // direction value the reference stores at (row, c): 0 diagonal, +length horizontal, -length vertical
    auto loadD = [&](int c, int row) -> int {
        if (row <= 0) return 1;   // D[c][0] = 1 (:118)
        if (!ok(c, row)) { left_band = true; return 0; }
        const unsigned nb = nibble(c, row);
        if ((nb & 3u) == 0u) return 0;
        int len = 1;
        if ((nb & 3u) == 1u) {
            unsigned f = nb;
            for (int x = c; (f & 4u) && x > 1;) {
                ++len; --x;
                if (!ok(x, row)) { left_band = true; break; }
                f = nibble(x, row);
            }
            return len;
        }
        unsigned f = nb;
        for (int y = row; (f & 8u) && y > 1;) {
            ++len; --y;
            if (!ok(c, y)) { left_band = true; break; }
            f = nibble(c, y);
        }
        return -len;
    };
    auto diag_run = [&](int c, int row) -> int {   // diagonal moves from (row, c) on, at most 64 (a cell without codes ends the run: the walk meets it next)
        const int rr = row - lane, cc = c - lane;
        const bool stop = !(rr >= 1 && cc >= 1) || !ok(cc, rr) || (nibble(cc, rr) & 3u) != 0u;
        const unsigned long long nd = __ballot(stop);
        return nd ? static_cast<int>(__builtin_ctzll(nd)) : 64;
    };
    int row = L, c = R;
    if (MODE == 1) {
        const unsigned long long map_words = (static_cast<unsigned long long>(R + 1) * 4 + sizeof(Word) - 1) / sizeof(Word);
        int32_t* const map = reinterpret_cast<int32_t*>(dirs + (A.dirs_per_wave - map_words));   // (behind the codes)
        while (c > 0) {
            const int run = diag_run(c, row);
            if (run > 0) {
                if (lane < run) map[c - lane] = (row - lane) * 2 + 1;
                row -= run; c -= run;
                continue;
            }
            const int d = loadD(c, row);
            if (left_band) return false;
            if (d < 0) { row += d; continue; }   // up moves leave the map untouched (:286)
            for (int x = lane; x < d && c - x > 0; x += 64) map[c - x] = (row + 1) * 2;
            c -= min(d, c);
        }
        __threadfence();
        if (lane == 0) {
            auto interval = [&](int a, int b, bool gaps, unsigned& st, unsigned& en) {   // (:307-351), size_t wrap kept via unsigned
                if (!gaps) {
                    st = map[a + 1] >> 1;
                    en = (map[b] >> 1) + (map[b] & 1);
                } else {
                    st = (a == 0) ? 1u : static_cast<unsigned>((map[a] >> 1) + (map[a] & 1));
                    en = (b + 1 == R + 1) ? static_cast<unsigned>(L + 1) : static_cast<unsigned>(map[b + 1] >> 1);
                }
                st -= 1;
                en -= 1;
            };
            unsigned st, en;
            interval(0, R, false, st, en);
            const bool nonempty = st < en;
            A.starts[read] = nonempty ? static_cast<int32_t>(st + 1) : 0;
            A.ends[read] = nonempty ? static_cast<int32_t>(en) : 0;
            for (int x = 0; x < A.nsec; ++x) {
                interval(A.sec_s[x], A.sec_e[x], true, st, en);
                A.sec_so[static_cast<long long>(x) * A.sec_stride + read] = static_cast<int32_t>(st + 1);
                A.sec_wo[static_cast<long long>(x) * A.sec_stride + read] = static_cast<int32_t>(en - st);
            }
        }
    } else {   // gapped strings, emitted from the end (:353-389)
        const long long base = start + read * static_cast<long long>(R);
        uint8_t* const oref = A.aln_ref + base;
        uint8_t* const oqry = A.aln_qry + base;
        const uint8_t* const sq = A.seq + start;
        int m = 0, ed = 0;
        while (c > 0) {
            const int run = diag_run(c, row);
            if (run > 0) {
                bool diff = false;
                if (lane < run) {
                    const uint8_t rc = A.refchars[c - 1 - lane], qc = sq[row - 1 - lane];
                    oref[m + lane] = rc; oqry[m + lane] = qc;
                    diff = rc != qc;
                }
                ed += static_cast<int>(__popcll(__ballot(diff)));
                m += run; row -= run; c -= run;
                continue;
            }
            const int d = loadD(c, row);
            if (left_band) return false;
            if (d < 0) {   // read bases opposite a gap
                for (int x = lane; x < -d; x += 64) { oref[m + x] = '-'; oqry[m + x] = sq[row - 1 - x]; }
                m -= d; ed -= d; row += d;
            } else {       // reference characters opposite a gap
                const int dd = min(d, c);
                for (int x = lane; x < dd; x += 64) { oref[m + x] = A.refchars[c - 1 - x]; oqry[m + x] = '-'; }
                m += dd; ed += dd; c -= dd;
            }
        }
        for (int x = lane; x < row; x += 64) { oref[m + x] = '-'; oqry[m + x] = sq[row - 1 - x]; }
        m += max(row, 0); ed += max(row, 0);
        if (lane == 0) { A.aln_len[read] = m; A.edits[read] = ed; }
    }
    return true;
}

// MODE 0 scores, 1 scores + map + sections, 2 scores + strings + edit distance.  PENSEL: the reference's penalty selects spelled
// out (needed when gapopen < 0).  Otherwise the "Penalty selection" argument of k_align applies cell for cell: a gap step out of
// a cell that was itself entered by the same kind of gap finds the running jump score equal to that cell's score, bit for bit,
// so with open >= extension max(jump - extension, score - open) is the double the reference computes either way, and its
// "jump continued" flag is the raw comparison AND NOT "that cell was entered by this kind of gap" -- both at hand here, so
// the codes, and the walk, are the same in both instantiations.
template <int K, int MODE, bool PENSEL, bool STRIPS>
__global__ void __launch_bounds__(WIDE_MAXT) k_align_wide(const AlignArgs A) {
    using Word = typename WideWord<K>::type;
    extern __shared__ __align__(16) unsigned char w_smem[];
    const int T = static_cast<int>(blockDim.x);
    const int t = static_cast<int>(threadIdx.x);
    const int R = A.R;
    // References of more than T K columns go through in STRIPS of T K columns, one after the other for every alignment: the last
    // column of a strip leaves its row state (score, running horizontal jump score, "was a horizontal gap") in a boundary array
    // in the workgroup's scratch, row by row, and the first thread of the next strip takes its left inputs from there (staged
    // WIDE_CH rows at a time like the read) instead of from DP column 0.  Codes: one tile per strip.
    const int CS = T * K;                                             // columns per strip
    const int nstrips = STRIPS ? (R + CS - 1) / CS : 1;               // (STRIPS = false: the instantiation for references of one strip, without the boundary code)
    double* const s_tab = reinterpret_cast<double*>(w_smem);
    double* const h_s = s_tab + A.tab_doubles;                        // [2][T] score handed to the next thread
    double* const h_lj = h_s + 2 * T;                                 // [2][T] running horizontal jump score
    double* const b_s = h_lj + 2 * T;                                 // [WIDE_CH] boundary rows staged for thread 0: score ...
    double* const b_lj = b_s + WIDE_CH;                               // ... jump score ...
    int* const h_fl = reinterpret_cast<int*>(b_lj + WIDE_CH);         // [2][T] the cell was a horizontal gap
    int* const b_fl = h_fl + 2 * T;                                   // [WIDE_CH] ... and flag
    uint16_t* const s_ring = reinterpret_cast<uint16_t*>(b_fl + WIDE_CH);   // [WIDE_RING]
    for (int e = t; e < A.tab_doubles; e += T) s_tab[e] = A.tables[e];
    const double NEG_INF = -__builtin_huge_val();
    const double GO = A.GO, GE = A.GE;
    const bool local = A.local != 0;
    const long long Rw = T;                        // words per step
    const long long strip_words = (static_cast<long long>(A.wide_maxlen) + T + 1) * Rw;
    Word* const dirs = MODE ? reinterpret_cast<Word*>(A.dirs) + static_cast<size_t>(blockIdx.x) * A.dirs_per_wave : nullptr;
    // boundary arrays of the workgroup (two sets, strips alternate): [2][3][longest read + 2] doubles
    const size_t bstride = static_cast<size_t>(A.wide_maxlen) + 2;
    double* const bnd = A.wide_bnd + static_cast<size_t>(blockIdx.x) * 6 * bstride;
    double Sc[K], Dg[K], UJ[K];
    for (long long read = blockIdx.x; read < A.n; read += gridDim.x) {
        const long long start = A.off[read];
        const int L = static_cast<int>(A.off[read + 1] - start);
        for (int st = 0; st < nstrips; ++st) {
        __syncthreads();
        const int col0 = st * CS;                                     // columns col0 + 1 .. col0 + Rs
        const int Rs = min(CS, R - col0);
        const int ncolv = max(0, min(K, Rs - t * K));                 // this thread's columns inside the strip
        const int tR = (Rs - 1) / K;
        const bool bnd_in = STRIPS && st > 0, bnd_out = STRIPS && st + 1 < nstrips;
        const double* const bi_s = bnd + static_cast<size_t>((st + 1) & 1) * 3 * bstride;   // written by the strip before
        double* const bo_s = bnd + static_cast<size_t>(st & 1) * 3 * bstride;
        Word* const sdirs = MODE ? dirs + st * strip_words : nullptr;
        int cb[K];
        unsigned upneg = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {   // DP row 0 of the thread's columns and of the column to their left
            const int col = min(col0 + t * K + k + 1, R);
            cb[k] = static_cast<int>(A.colbase[col]);
            Sc[k] = A.rowzero[col]; Dg[k] = A.rowzero[col - 1]; UJ[k] = NEG_INF;
        }
        const int nsteps = L > 0 ? L + tR : 0;   // thread tR finishes row L at step L + tR
        for (int s = 1; s <= nsteps; ++s) {
            if ((s - 1) % WIDE_CH == 0) {   // rows s .. s + WIDE_CH - 1 into the ring (thread 0 needs row s now)
                for (int e = t; e < WIDE_CH; e += T) {
                    const int row = s + e;
                    uint32_t ent = 0;
                    if (row <= L) {
                        const long long idx = start + row - 1;
                        int qi = static_cast<int>(static_cast<signed char>(A.qual[idx])) - A.qoffset;
                        if (qi < 0) atomicMin(A.badqual, A.read_base + static_cast<int>(read));
                        qi = qi < 0 ? 0 : (qi >= A.navail ? A.navail - 1 : qi);
                        uint32_t code;
                        if (A.nmask) {
                            code = ((A.nmask[idx >> 3] >> (idx & 7)) & 1u) ? 4u : ((A.seq[idx >> 2] >> ((idx & 3) * 2)) & 3u);
                        } else {
                            const uint32_t b = A.seq[idx];
                            code = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
                        }
                        ent = code * static_cast<uint32_t>(A.row_bytes) + static_cast<uint32_t>(qi << 3);
                        if (bnd_in) {   // the row state the strip before left in its last column
                            b_s[e] = bi_s[row]; b_lj[e] = bi_s[bstride + row];
                            b_fl[e] = static_cast<int>(reinterpret_cast<const long long*>(bi_s + 2 * bstride)[row]);
                        }
                    }
                    s_ring[row & (WIDE_RING - 1)] = static_cast<uint16_t>(ent);
                }
                __syncthreads();
            }
            const int i = s - t;
            const int par = s & 1;
            if (i >= 1 && i <= L && ncolv > 0) {
                double ls, lj;
                bool lpos;
                if (t == 0) {
                    if (bnd_in) {   // (thread 0 is at row s: entry (s - 1) % WIDE_CH of the staged boundary rows)
                        const int e = (i - 1) % WIDE_CH;
                        ls = b_s[e]; lj = b_lj[e]; lpos = b_fl[e] != 0;
                    } else {        // DP column 0 (src/reference_align.cpp:63-78)
                        ls = local ? 0.0 : (-GO - GE * static_cast<double>(i - 1));
                        lj = NEG_INF;
                        lpos = false;
                    }
                } else {
                    ls = h_s[(par ^ 1) * T + t - 1];
                    lj = h_lj[(par ^ 1) * T + t - 1];
                    lpos = h_fl[(par ^ 1) * T + t - 1] != 0;
                }
                const int ent = s_ring[i & (WIDE_RING - 1)];
                Word w = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (k < ncolv) {
                        const bool lastcol = local && (col0 + t * K + k + 1 == R);   // free vertical gaps in the last column (:93)
                        const double vgo = lastcol ? 0.0 : GO, vge = lastcol ? 0.0 : GE;
                        const bool upn = ((upneg >> k) & 1u) != 0u;
                        double horiz, vert;
                        bool hc, vc;
                        if (PENSEL) {
                            horiz = ls - (lpos ? GE : GO);
                            lj -= GE;
                            hc = lj > horiz;
                            if (hc) horiz = lj; else lj = horiz;
                            vert = Sc[k] - (upn ? vge : vgo);
                            double uj = UJ[k] - vge;
                            vc = uj > vert;
                            if (vc) vert = uj; else uj = vert;
                            UJ[k] = uj;
                        } else {
                            const double hopen = ls - GO, vopen = Sc[k] - vgo;
                            lj -= GE;
                            hc = lj > hopen && !lpos;
                            horiz = fmax(lj, hopen);
                            lj = horiz;
                            const double uj = UJ[k] - vge;
                            vc = uj > vopen && !upn;
                            vert = fmax(uj, vopen);
                            UJ[k] = vert;
                        }
                        const double cost = *reinterpret_cast<const double*>(reinterpret_cast<const unsigned char*>(s_tab) + cb[k] + ent);
                        const double match = Dg[k] + cost;
                        Dg[k] = ls;
                        // (:164-177) the diagonal if it beats both gaps, else the horizontal gap if it beats the vertical one; the score is
                        // the maximum of the three either way (no NaN, no -0 on this path: the selected operand bit for bit)
                        const double hv = fmax(horiz, vert);
                        const double cur = fmax(match, hv);
                        const unsigned kind = match > hv ? 0u : (horiz > vert ? 1u : 2u);
                        Sc[k] = cur;
                        upneg = (upneg & ~(1u << k)) | ((kind == 2u ? 1u : 0u) << k);
                        ls = cur;
                        lpos = kind == 1u;
                        if (MODE) w |= static_cast<Word>(kind | (hc ? 4u : 0u) | (vc ? 8u : 0u)) << (4 * (K - 1 - k));   // (column k in nibble K - 1 - k: what k_align_wide_q's bit pushes leave)
                    }
                }
                h_s[par * T + t] = ls;
                h_lj[par * T + t] = lj;
                h_fl[par * T + t] = lpos ? 1 : 0;
                if (bnd_out && t == tR) {   // the strip's last column: its row state for the next strip
                    bo_s[i] = ls; bo_s[bstride + i] = lj;
                    reinterpret_cast<long long*>(bo_s + 2 * bstride)[i] = lpos ? 1 : 0;
                }
                if (MODE) __builtin_nontemporal_store(w, &sdirs[static_cast<long long>(s) * Rw + t]);
            }
            __syncthreads();
        }
        if (bnd_out) __threadfence();
        if (st + 1 < nstrips) continue;
        const int kR = (Rs - 1) % K;
        if (t == tR) {
            double sc = Sc[0];
#pragma unroll
            for (int k = 1; k < K; ++k) sc = (k == kR) ? Sc[k] : sc;
            if (L == 0) sc = A.rowzero[R];   // no rows: row 0 of the last column (:115-118)
            A.scores[read] = sc;
        }
        if (MODE) {
            __threadfence();
            __syncthreads();
            if (t < 64) (void)wide_walk<K, MODE, STRIPS>(A, dirs, strip_words, CS, Rw, L, R, read, start, t);
        }
        }   // (strips)
    }
}

// ---------------------------------------------------------------------------
// k_align_wide_q: the same alignment without a barrier per step (global mode, gapopen >= 0, one strip: the qualityAlign shape).
// k_align_wide hands the row state from thread to thread through LDS with one workgroup barrier per step; measured at 2 kb x
// 2 kb the vector units idle half of the time -- every step is a round trip LDS write -> barrier -> LDS read in front of a
// chain of 8 dependent cells.  Here a WAVEFRONT is the unit: inside it the row state goes to the next lane with DPP moves
// (wave_shr:1, lane 0 keeps the fill operand), exactly as in k_align, and only between consecutive wavefronts does it go
// through LDS -- a queue of WQ_B rows per wavefront boundary, filled by lane 63 of the producer and read by lane 0 of the
// consumer, which runs 64 rows behind by construction.  The two look at each other's progress counters once per WQ_SYNC
// steps (consumer: "are my next WQ_SYNC rows there", producer: "are the slots of my next WQ_SYNC rows free") and otherwise
// run freely; every wait is bounded and sets the abort flag, which every wavefront sees at its next look, so the grid drains
// whatever happens.  Read rows are staged per wavefront, 64 at a time one refill ahead, in a 128-entry ring (k_align's
// scheme).  All flags are lane masks in scalar registers, inactive lanes (ramp-up and ramp-down of the skew) are switched
// off by EXEC alone.  Codes, tile layout and walk are k_align_wide's.
constexpr int WQ_B = 128;       // rows of a queue (power of two; producer and consumer are 64 rows apart + WQ_SYNC of slack each way)
constexpr int WQ_SYNC = 16;     // steps between two looks at the neighbours' progress
constexpr int WQ_SPINS = 1 << 22;
constexpr int WIDE_BAND = 96;   // rows either side of the main diagonal whose cells carry codes in the first launch (reads with 1 % indel events drift by a few dozen)

__device__ __forceinline__ int wq_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void wq_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
// wait until *p >= need; false: gave up (another wavefront did, or the bound was reached) -- the caller leaves its loop
__device__ __forceinline__ bool wq_wait(const int* p, int need, int* abort_flag) {
    for (int spins = 0; wq_load(p) < need; ++spins) {
        if (wq_load(abort_flag) != 0 || spins > WQ_SPINS) { wq_store(abort_flag, 1); return false; }
        __builtin_amdgcn_s_sleep(2);
    }
    return true;
}
__device__ __forceinline__ double dpp_wave_shr1(double v, double lane0) {
    const int hi = __builtin_amdgcn_update_dpp(hi32(lane0), hi32(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const int lo = __builtin_amdgcn_update_dpp(lo32(lane0), lo32(v), 0x138, 0xf, 0xf, false);
    return mk64(hi, lo);
}

// v_max_f64 as the instruction itself: fmax() of a value that arrives through a loop-carried register makes the compiler
// canonicalise it first (one more v_max_f64 x, x, x per use), which costs what carrying the value saves; what follows a
// raw maximum in the chain of a cell is raw too.  (No NaN reaches these: maximum of two numbers, bit for bit the greater.)
__device__ __forceinline__ double max_f64_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int K, int MODE>
__global__ void __launch_bounds__(WIDE_MAXT) k_align_wide_q(const AlignArgs A) {
    using Word = typename WideWord<K>::type;
    extern __shared__ __align__(16) unsigned char w_smem[];
    const int T = static_cast<int>(blockDim.x);
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int NWV = T >> 6;
    // Which 512 columns a wavefront takes is rotated from workgroup to workgroup: hardware wavefront h of every workgroup sits on
    // SIMD h mod 4, and with the codes confined to a band the wavefronts near the diagonal have more to issue than the others --
    // without the rotation the four SIMDs of a CU take turns at being the busy one.  `wv` and `t` are the LOGICAL indices (the
    // wavefront's position along the reference, the thread's position among the column owners) everywhere below.
    const int hw = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int wv = (hw + static_cast<int>((blockIdx.x * 2654435761u) >> 16)) % NWV;
    const int t = wv * 64 + lane;
    const int R = A.R;
    double* const s_tab = reinterpret_cast<double*>(w_smem);
    double* const q_s = s_tab + A.tab_doubles;                          // [NWV][WQ_B] score of a wavefront's last column, by row
    double* const q_lj = q_s + NWV * WQ_B;                              // ... its running horizontal jump score
    int* const q_fl = reinterpret_cast<int*>(q_lj + NWV * WQ_B);        // ... "that cell was a horizontal gap"
    int* const s_prog = q_fl + NWV * WQ_B;                              // [NWV] rows a wavefront's lane 63 has written
    int* const s_cons = s_prog + NWV;                                   // [NWV] rows a wavefront's lane 0 has taken
    int* const s_abort = s_cons + NWV;                                  // [1] (+ padding)
    uint16_t* const s_ring = reinterpret_cast<uint16_t*>(s_abort + 2) + wv * 128;   // [NWV][128] staged read rows of this wavefront
    for (int e = t; e < A.tab_doubles; e += T) s_tab[e] = A.tables[e];
    const double NEG_INF = -__builtin_huge_val();
    const double GO = A.GO, GE = A.GE;
    Word* const dirs = MODE ? reinterpret_cast<Word*>(A.dirs) + static_cast<size_t>(blockIdx.x) * A.dirs_per_wave : nullptr;
    const int tR = (R - 1) / K, kR = (R - 1) % K;
    // (threads beyond column R -- the spare columns of thread tR, the padding of the last wavefront -- compute on column R's
    // tables values nobody reads)
    const bool has_next = wv + 1 < NWV;
    int cb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cb[k] = static_cast<int>(A.colbase[min(t * K + k + 1, R)]);
    const unsigned char* const tabb = reinterpret_cast<const unsigned char*>(s_tab);
    // Per column: Sg = score of the row above MINUS the opening penalty (what the vertical candidate of this row and the
    // horizontal candidate of the next column both are: one subtraction per cell serves both), Dg = score of the column to the
    // left in the row above (this row's diagonal), UJ = running vertical jump score.
    double Sg[K], Dg[K], UJ[K];
    // the reads of this launch: 0 .. n - 1, or (the launch behind a banded one) the reads whose walks left the band
    const long long nwork = A.wide_list ? static_cast<long long>(A.wide_list[-1]) : A.n;
    for (long long item = blockIdx.x; item < nwork; item += gridDim.x) {
        const long long read = A.wide_list ? static_cast<long long>(A.wide_list[item]) : item;
        const long long start = A.off[read];
        const int L = static_cast<int>(A.off[read + 1] - start);
        __syncthreads();   // (the walk of the alignment before is done with the tile; the tables are in place)
        if (lane == 0) { s_prog[wv] = 0; s_cons[wv] = 0; }
        if (t == 0) *s_abort = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {   // DP row 0 of the thread's columns and of the column to their left
            const int col = min(t * K + k + 1, R);
            Sg[k] = A.rowzero[col] - GO; Dg[k] = A.rowzero[col - 1]; UJ[k] = NEG_INF;
        }
        double ls_out = 0.0, lj_out = NEG_INF;
        double final_score = A.rowzero[R];   // (no rows: row 0 of the last column, :115-118)
        // A read row is requested one refill (64 steps) before it is staged: the loads (quality byte, base byte or its two packed
        // bytes) are issued and left in flight, the entry -- byte offset inside a column's cost rows -- is made from them when the
        // ring takes it, so no step waits for memory.
        struct RawRow { uint32_t q, b, m; };
        auto request_row = [&](int row) -> RawRow {
            RawRow r{0u, 0u, 0u};
            if (row > L) return r;
            const long long idx = start + row - 1;
            r.q = A.qual[idx];
            if (A.nmask) { r.m = A.nmask[idx >> 3]; r.b = A.seq[idx >> 2]; }
            else r.b = A.seq[idx];
            return r;
        };
        auto entry_of = [&](const RawRow& r, int row) -> uint32_t {
            if (row > L) return 0u;
            const long long idx = start + row - 1;
            int qi = static_cast<int>(static_cast<signed char>(r.q)) - A.qoffset;
            if (qi < 0) atomicMin(A.badqual, A.read_base + static_cast<int>(read));
            qi = qi < 0 ? 0 : (qi >= A.navail ? A.navail - 1 : qi);
            uint32_t code;
            if (A.nmask) code = ((r.m >> (idx & 7)) & 1u) ? 4u : ((r.b >> ((idx & 3) * 2)) & 3u);
            else code = r.b == 'A' ? 0u : r.b == 'C' ? 1u : r.b == 'G' ? 2u : r.b == 'T' ? 3u : 4u;
            return code * static_cast<uint32_t>(A.row_bytes) + static_cast<uint32_t>(qi << 3);
        };
        RawRow pf = request_row(1 + lane);
        const int nsteps = L > 0 ? L + 63 : 0;   // lane 63 finishes row L at step L + 62
        // Codes for the cells near the main diagonal only (wide_band > 0): the steps [c_lo, c_hi] of this wavefront.  Outside them
        // a step still takes the two comparisons that say which move a cell made -- the flags the next row, the next column and the
        // next wavefront take from it stay right everywhere -- but not the two jump comparisons, the four bit pushes and the store.
        const WideBand wband{MODE ? A.wide_band : 0, L, R};
        const bool banded = MODE != 0 && A.wide_band > 0;
        const int c_lo = banded ? wband.lo(wv) : 0, c_hi = banded ? wband.hi(wv) : 0x7fffffff;
        bool aborted = false;
        // what every step starts with: the ring refill and, every WQ_SYNC steps, the look at the neighbours; false: give up
        auto step_head = [&](int sg) -> bool {
            if ((sg & 63) == 0) {   // rows sg + 1 .. sg + 64 into the ring (lane 0 needs row sg + 1 now); the next 64 requested
                s_ring[(sg + lane) & 127] = static_cast<uint16_t>(entry_of(pf, sg + 1 + lane));
                pf = request_row(sg + 65 + lane);
            }
            if ((sg & (WQ_SYNC - 1)) == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (lane 63's queue entries of the steps before, in front of the counters)
                int ok = 1;
                if (lane == 0) {
                    // what this wavefront has taken and written so far -- published before it waits for anybody
                    wq_store(&s_cons[wv], min(sg, L));
                    wq_store(&s_prog[wv], min(max(sg - 63, 0), L));
                    if (wv > 0) ok = wq_wait(&s_prog[wv - 1], min(L, sg + WQ_SYNC), s_abort) ? 1 : 0;                    // my next rows are there
                    if (ok && has_next) ok = wq_wait(&s_cons[wv + 1], min(L, sg - 47) - WQ_B, s_abort) ? 1 : 0;         // the slots of my next rows are free
                    if (wq_load(s_abort) != 0) ok = 0;
                }
                ok = __builtin_amdgcn_readfirstlane(ok);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (!ok) return false;
            }
            return true;
        };
        // the row state of the column to lane 0's left at step sg (row sg + 1): DP column 0 (first wavefront,
        // src/reference_align.cpp:63-78, global mode) or the queue of the wavefront before
        auto lane0_in = [&](int sg, double& l0, double& j0, int& f0) {
            if (wv == 0) {
                l0 = -GO - GE * static_cast<double>(sg);   // -GO - GE (i - 1)
                j0 = NEG_INF;
                f0 = 0;
            } else {
                const int e = (wv - 1) * WQ_B + (sg & (WQ_B - 1));   // row sg + 1 sits in slot (row - 1) mod WQ_B
                l0 = q_s[e]; j0 = q_lj[e];
                f0 = MODE ? q_fl[e] : 0;
            }
        };

        // ---- steps 0 .. 62: the lanes enter the read one by one.  Per-lane flags, the cells under `if (active)` (a lane that has
        // not entered keeps DP row 0 in its columns; also every step of a read of fewer than 64 rows' start) ----
        unsigned upneg = 0;      // bit k: the move of column k's cell in the row above was a vertical gap (row 0: no)
        int lpos_out = 0;        // my last column's cell was a horizontal gap, of the step before
        int sg = 0;
        for (; sg < min(nsteps, 63); ++sg) {
            if (!step_head(sg)) { aborted = true; break; }
            const int i = sg - lane + 1;
            const bool active = i >= 1 && i <= L;
            double l0, j0;
            int f0;
            lane0_in(sg, l0, j0, f0);
            double ls = dpp_wave_shr1(ls_out, l0);
            double lj = dpp_wave_shr1(lj_out, j0);
            bool lpos = __builtin_amdgcn_update_dpp(f0, lpos_out, 0x138 /* wave_shr:1 */, 0xf, 0xf, false) != 0;
            if (active) {
                const int ent = s_ring[(sg - lane) & 127];
                uint32_t w = 0;
                double hopen = ls - GO;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double vopen = Sg[k];
                    const double ljm = lj - GE;
                    const bool hc = ljm > hopen && !lpos;
                    const double horiz = fmax(ljm, hopen);
                    lj = horiz;
                    const double ujm = UJ[k] - GE;
                    const bool vc = ujm > vopen && ((upneg >> k) & 1u) == 0u;
                    const double vert = max_f64_raw(ujm, vopen);
                    UJ[k] = vert;
                    const double match = Dg[k] + *reinterpret_cast<const double*>(tabb + cb[k] + ent);
                    Dg[k] = ls;
                    const double hv = max_f64_raw(horiz, vert);
                    const double cur = max_f64_raw(match, hv);
                    const unsigned kind = match > hv ? 0u : (horiz > vert ? 1u : 2u);
                    upneg = (upneg & ~(1u << k)) | ((kind == 2u ? 1u : 0u) << k);
                    lpos = kind == 1u;
                    if (MODE) w |= static_cast<uint32_t>(kind | (hc ? 4u : 0u) | (vc ? 8u : 0u)) << (4 * (K - 1 - k));
                    ls = cur;
                    hopen = cur - GO;
                    Sg[k] = hopen;
                    if (t == tR && i == L && k == kR) final_score = cur;   // (a read of fewer than 64 rows can end here)
                }
                ls_out = ls;
                lj_out = lj;
                lpos_out = lpos ? 1 : 0;
                if (MODE) __builtin_nontemporal_store(static_cast<Word>(w), &dirs[static_cast<long long>(i + t) * T + t]);
                if (has_next && lane == 63) {
                    const int e = wv * WQ_B + ((i - 1) & (WQ_B - 1));
                    q_s[e] = ls; q_lj[e] = lj;
                    if (MODE) q_fl[e] = lpos ? 1 : 0;
                }
            }
        }

        // ---- steps 63 .. L + 62: every lane has entered.  Nothing in the cells is predicated and every flag is a wave-uniform
        // lane mask in scalar registers.  A lane past row L computes all the same; what it computes is never used: codes and
        // queue entries are stored for rows 1 .. L only, the score is taken at row L, and nobody takes the outputs of a lane
        // that is not at a row of the read. ----
        mask_t m_up[K];
#pragma unroll
        for (int k = 0; k < K; ++k) m_up[k] = MODE ? __builtin_amdgcn_ballot_w64(((upneg >> k) & 1u) != 0u) : 0;
        mask_t m_lp_out = MODE ? __builtin_amdgcn_ballot_w64(lpos_out != 0) : 0;
        // (three loops -- before, inside and behind the steps that carry codes -- rather than one loop with both versions of the cells:
        // with both in one loop the allocator spilled in the cells, 65 -> 102 ms)
        auto main_steps = [&](auto coded_tag, int s_end) {
          constexpr bool CODED = decltype(coded_tag)::value;
          for (; !aborted && sg < s_end; ++sg) {
            if (!step_head(sg)) { aborted = true; break; }
            const int i = sg - lane + 1;
            const bool active = i <= L;
            double l0, j0;
            int f0;
            lane0_in(sg, l0, j0, f0);
            double ls = dpp_wave_shr1(ls_out, l0);
            double lj = dpp_wave_shr1(lj_out, j0);
            mask_t m_lp = (m_lp_out << 1) | (MODE ? (__builtin_amdgcn_ballot_w64(f0 != 0) & 1ull) : 0ull);
            const int ent = s_ring[(sg - lane) & 127];   // (a lane past the read finds the 0 the refill staged for rows beyond L: a valid table address)
            uint32_t w = 0;
            double cost[K], curs[K];
#pragma unroll
            for (int k = 0; k < K; ++k) cost[k] = *reinterpret_cast<const double*>(tabb + cb[k] + ent);   // (requested back to back, ahead of the chain of cells)
            {
                double hopen = ls - GO;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    // (src/reference_align.cpp:125-177 without the penalty selects: see k_align's "Penalty selection")
                    const double vopen = Sg[k];
                    const double ljm = lj - GE;
                    const mask_t m_hcr = CODED ? __builtin_amdgcn_ballot_w64(ljm > hopen) : 0;
                    const double horiz = fmax(ljm, hopen);
                    lj = horiz;
                    const double ujm = UJ[k] - GE;
                    const mask_t m_vcr = CODED ? __builtin_amdgcn_ballot_w64(ujm > vopen) : 0;
                    const double vert = max_f64_raw(ujm, vopen);
                    UJ[k] = vert;
                    const double match = Dg[k] + cost[k];
                    Dg[k] = ls;
                    const double hv = max_f64_raw(horiz, vert);
                    const double cur = max_f64_raw(match, hv);
                    if (MODE) {
                        const mask_t m_tm = __builtin_amdgcn_ballot_w64(match > hv), m_hv = __builtin_amdgcn_ballot_w64(horiz > vert);
                        const mask_t m_k1 = m_hv & ~m_tm, m_k2 = ~(m_hv | m_tm);   // horizontal gap / vertical gap (neither: diagonal)
                        if (CODED) {
                            const mask_t m_hc = m_hcr & ~m_lp, m_vc = m_vcr & ~m_up[k];   // the jumps really continued
                            w = push_bit(push_bit(push_bit(push_bit(w, m_vc), m_hc), m_k2), m_k1);   // column k ends up in nibble K - 1 - k
                        }
                        m_lp = m_k1;
                        m_up[k] = m_k2;
                    }
                    curs[k] = cur;
                    ls = cur;
                    hopen = cur - GO;   // the next column's horizontal candidate and, one step on, this column's vertical one
                    Sg[k] = hopen;
                }
            }
            ls_out = ls;
            lj_out = lj;
            if (MODE) m_lp_out = m_lp;
            if (sg == L - 1 + (tR & 63) && wv == NWV - 1) {   // thread tR is at row L: the score (one step of one wavefront)
                double sc = curs[0];
#pragma unroll
                for (int k = 1; k < K; ++k) sc = (k == kR) ? curs[k] : sc;
                if (t == tR) final_score = sc;
            }
            if (active) {
                // (word of thread t at its step i + t = sg + 1 + 64 wv, the same for every lane: a scalar row address + the lane's offset)
                if (MODE && CODED) __builtin_nontemporal_store(static_cast<Word>(w), dirs + static_cast<long long>(sg + 1 + 64 * wv) * T + t);
                if (has_next && lane == 63) {   // my last column's row state for the wavefront after me
                    const int e = wv * WQ_B + ((i - 1) & (WQ_B - 1));
                    q_s[e] = ls; q_lj[e] = lj;
                    if (MODE) q_fl[e] = static_cast<int>((m_lp >> 63) & 1ull);
                }
            }
          }
        };
        if (MODE != 0) main_steps(Flag<false>{}, min(nsteps, c_lo));
        main_steps(Flag<MODE != 0>{}, c_hi < nsteps - 1 ? c_hi + 1 : nsteps);
        if (MODE != 0) main_steps(Flag<false>{}, nsteps);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) { wq_store(&s_cons[wv], L); wq_store(&s_prog[wv], aborted ? 0 : L); }
        if (aborted && lane == 0) atomicExch(A.badqual + 1, 1);
        if (t == tR) A.scores[read] = final_score;
        if (MODE) {
            __threadfence();
            __syncthreads();
            if (t < 64 && wq_load(s_abort) == 0) {
                const bool done = wide_walk<K, MODE, false>(A, dirs, 0, T * K, T, L, R, read, start, t, banded ? &wband : nullptr);
                if (!done && t == 0) A.wide_redo[1 + atomicAdd(A.wide_redo, 1)] = static_cast<int>(read);   // again, with the codes of every cell
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host side

// MODE 4 (see LOC_NEG): the integer tables and the constants of the exactness argument, or false when the call is not
// eligible (it then runs MODE 3): GE > 0, gapopen >= 0, GO 2^k and GE 2^k integers, and an integer range that fits.
struct LocPlan {
    std::vector<int> tab, rz;
    int k = 0, GO = 0, GE = 0, D = 0;
    double unit = 0, slack = 0, top = 0;
    bool framed = false;   // tab, rz and GO are those of the extension-free frame (MODE 6)
};
static bool plan_locate(const std::vector<double>& rows, const std::vector<uint32_t>& colbase, int n, int R, double GO,
                        double GE, const std::vector<double>& rowzero, int64_t max_len, int frame, LocPlan& p) {
    if (!(GE > 0) || !(GO >= GE) || !std::isfinite(GO) || R < 1) return false;
    double splus = 0, wmax = 0;   // sum over columns of max(0, largest entry); largest finite |entry|
    for (double v : rows) {
        if (std::isnan(v) || v == std::numeric_limits<double>::infinity()) return false;
        if (std::isfinite(v)) wmax = std::max(wmax, std::fabs(v));
    }
    for (int col = 1; col <= R; ++col) {
        double smax = 0;
        const size_t b = colbase[col] / sizeof(double);
        for (size_t x = 0; x < static_cast<size_t>(5 * n); ++x) smax = std::max(smax, rows[b + x]);
        splus += smax;
    }
    double rzplus = 0, rzmag = 0;
    for (double v : rowzero) { rzplus = std::max(rzplus, v); rzmag = std::max(rzmag, std::fabs(v)); }
    const double bneg = GO + GE * R + rzmag;   // every cell is >= -bneg (the horizontal path from column 0, or row 0)
    const double bpos = splus + rzplus;        // ... and <= bpos
    const double bmag = std::max(bneg, bpos) + wmax + GO;   // largest intermediate of a chain whose values are cells
    // a chain of cells falls by at most 2 bpos + bneg in all, at least GE per vertical step
    const double nops = 2.0 * R + 4.0 + (2.0 * bpos + bneg) / GE;
    const double eps = 2.0 * nops * bmag * std::ldexp(1.0, -53);
    // any chain of the window certificate, at most 2 (max_len + R) operations on values above -(bmag + GE max_len)
    const double lenx = static_cast<double>(max_len) + R + 2.0;
    const double eps_alt = 2.0 * 2.0 * lenx * (bmag + GE * lenx) * std::ldexp(1.0, -53);
    if (!(eps + eps_alt < 0.25)) return false;
    // largest k whose range (with the margin D ~ R + 3 units) stays below 2^27 in magnitude
    int k = 24;
    while (k > 0 && (bmag + GE) * std::ldexp(1.0, k) + 2.0 * (R + 4) > std::ldexp(1.0, 27)) --k;
    if ((bmag + GE) * std::ldexp(1.0, k) + 2.0 * (R + 4) > std::ldexp(1.0, 27)) return false;
    double go = std::ldexp(GO, k), ge = std::ldexp(GE, k);
    if (go != std::floor(go) || ge != std::floor(ge)) return false;   // not dyadic at this k: nor at any smaller one
    // The extension-free frame (MODE 6) adds GE 2^k (i + c) to cell (i, c): the largest k <= the one above whose framed
    // values and intermediates stay within 2^30, (bmag + GE (max_len + R + 2)) 2^k + 2 (R + 4) <= 2^30.  Un-framed values
    // stay above -2^27 as before (k only shrinks) and the frame adds nothing negative, so LOC_NEG keeps its place below
    // them.  The penalties must stay integers at that k; below LOC_FRAME_KMIN the un-framed locator runs at the k above.
    // frame: 1 as above, 0 never, 2 the un-framed locator at the frame's k (A/B of the frame alone)
    if (frame) {
        int kf = k;
        while (kf >= LOC_FRAME_KMIN && (bmag + GE * lenx) * std::ldexp(1.0, kf) + 2.0 * (R + 4) > std::ldexp(1.0, 30)) --kf;
        const double gof = std::ldexp(GO, kf), gef = std::ldexp(GE, kf);
        if (kf >= LOC_FRAME_KMIN && gof == std::floor(gof) && gef == std::floor(gef)) {
            p.framed = frame == 1;
            k = kf; go = gof; ge = gef;
        }
    }
    p.k = k;
    p.GO = static_cast<int>(go);
    p.GE = static_cast<int>(ge);
    p.tab.resize(rows.size());
    for (size_t x = 0; x < rows.size(); ++x)
        p.tab[x] = std::isfinite(rows[x]) ? static_cast<int>(std::nearbyint(std::ldexp(rows[x], k))) : LOC_NEG;
    p.rz.resize(rowzero.size());
    for (size_t x = 0; x < rowzero.size(); ++x) p.rz[x] = static_cast<int>(std::nearbyint(std::ldexp(rowzero[x], k)));
    if (p.framed) {   // a diagonal move crosses two anti-diagonals of the frame, an opening pays GO - GE, row 0 is GE c up
        for (int& v : p.tab) v = v == LOC_NEG ? LOC_NEG_FRAMED : v + 2 * p.GE;
        for (size_t x = 0; x < p.rz.size(); ++x) p.rz[x] += p.GE * static_cast<int>(x);
        p.GO -= p.GE;
    }
    p.D = (R + 1) + static_cast<int>(std::ceil(2.0 * eps * std::ldexp(1.0, k))) + 1;
    p.unit = std::ldexp(1.0, -k);
    p.slack = (R + 1) * std::ldexp(1.0, -(k + 1)) + eps;
    p.top = bpos + 1.0;
    return true;
}

struct Shape { int K, W, ngroups, rowf; };   // rowf: see k_align's ROWF

// Columns per lane / lanes per alignment / alignments per wave for a reference
// of R columns: maximise busy lanes, prefer more columns per lane on ties (fewer
// cross-lane moves per cell).
static Shape pick_shape(int R) {
    Shape best{1, 64, 1, 0};
    double best_u = -1;
    for (int K : {1, 2, 4, 8, 16}) {
        int W = (R + K - 1) / K;
        if (W > 64) continue;
        // groups of up to 16 lanes are padded to one DPP row: NGMAX = 4 of them fill the wave
        // and the leaders get their column-0 inputs for free (lane_shr1<1>)
        if (W <= 16) W = 16;
        const int ng = std::min(64 / W, NGMAX);
        const double u = static_cast<double>(ng) * R / (64.0 * K);
        if (u > best_u + 1e-9 || (u > best_u - 1e-9 && K > best.K && K <= 2)) { best_u = u; best = {K, W, ng, W == 16 ? 1 : 0}; }
    }
    // references of up to 32 columns: eight alignments of 8 lanes, two interleaved per DPP row (lane_shr1<2>) -- the
    // same share of busy lanes as four alignments of 16 lanes with half the columns per lane, and half the
    // cross-lane moves per cell
    for (int K : {2, 4}) {
        if ((R + K - 1) / K > 8) continue;
        const double u = static_cast<double>(NGMAX2) * R / (64.0 * K);
        if (u > best_u - 1e-9) { best_u = u; best = {K, 8, NGMAX2, 2}; break; }
    }
    return best;
}

// Everything a call decides before it touches the device
struct AlignPlan {
    double GO = 0, GE = 0;
    std::vector<double> rows, rowzero;   // the call's tables on the host: cost rows (build_cost_rows), DP row 0
    std::vector<uint32_t> colbase;
    Shape sh{1, 64, 1, 0};
    int klast = -1;   // index of column R inside its lane where k_align knows it at compile time (KLAST), else -1
    int mode = 0;   // the kernels': 0 scores, 1 / 2 the code stream (map / strings), 3 snapshots, 4 locator + window
    bool pensel = false, wide = false, classes = false, wide_queue = false;   // wide_queue: k_align_wide by k_align_wide_q
    size_t per_wave = 0, word_bytes = 4, lds = 0, redo_per_wave = 0;   // traceback tile of one wavefront (wide: of one workgroup), in words; LDS bytes
    long long grid = 0;
    // MODE 4: the locator's own launch shape, KLAST and grid (the window and snapshot launches run in `sh`)
    Shape loc_sh{1, 64, 1, 0};
    int loc_klast = -1;
    long long loc_grid = 0;
    int win_nb = 0, redo_grid = 0;   // window classes: the tiles (redo_per_wave) and the grid of the two small snapshot launches
    int wide_T = 0, wide_strips = 0, wide_band = 0;   // k_align_wide: threads, strips, see AlignArgs::wide_band
};

// Far more workgroups than fit at once: each wave then owns only a few work items and the
// hardware hands out workgroups as CUs free up, which balances the load much better than an
// exactly resident grid with a static stride (1.74 -> 2.07 TCUPS at 1M x 2kb; flat from 128 to
// 384 waves per CU).  The per-wave scratch tiles scale with the grid and are capped by the caller.
long long align_grid(long long nitems, int waves, int num_cu) {
    int waves_per_cu = 128;
    if (option(OPT_ALIGN_WAVES_PER_CU) > 0) waves_per_cu = option(OPT_ALIGN_WAVES_PER_CU);
    return std::min<long long>((nitems + waves - 1) / waves, (static_cast<long long>(num_cu) * waves_per_cu + waves - 1) / waves);
}

constexpr int WIDE_K = 8;   // (12 or 16 columns per thread at 2 kb: 3 x slower -- the unrolled columns spill at the 128 registers a 1 024-thread bound leaves)
// References beyond MAX_REF columns: one workgroup per alignment (k_align_wide).
static int plan_wide(const AlignJob& job, int num_cu, AlignPlan& p) {
    constexpr int K = WIDE_K;
    const int R = job.R, kernel_mode = p.mode == 3 ? 1 : p.mode;
    const int32_t max_len = job.batch.max_len;
    if (R > (1 << 20)) return fail("sarlacc_amd: reference longer than %d columns is not supported", 1 << 20);
    if (kernel_mode == 2 && job.batch.d_nmask) return fail("sarlacc_amd: alignment strings need ASCII reads");
    // up to 8 192 columns one strip of as many threads as the columns need; beyond, strips of 1 024 threads x 8 columns
    const int T = R <= K * WIDE_MAXT ? ((R + K - 1) / K + 63) / 64 * 64 : WIDE_MAXT;
    const int nstrips = (R + T * K - 1) / (T * K);
    const size_t word = 4;
    size_t per_wg = 0;   // words: codes of every step of every strip, then the reference -> read map
    if (kernel_mode) per_wg = static_cast<size_t>(nstrips) * (static_cast<size_t>(max_len) + T + 1) * T + ((static_cast<size_t>(R) + 1) * 4 + word - 1) / word;
    long long grid = std::min<long long>(job.batch.n, static_cast<long long>(num_cu) * std::max(1, 2048 / T));
    if (kernel_mode) {
        const size_t budget = static_cast<size_t>(16) << 30;
        // (4 bits per cell of the whole matrix per alignment in flight: a 2^20-column reference against 100-kb reads would be 50 GB)
        if (per_wg * word > budget)
            return fail("sarlacc_amd: the traceback of one alignment of %d reference columns against reads of up to %d bases needs %.1f GB "
                        "of scratch (at most 16): ask for scores only (barcode_align) or align shorter pieces", R, max_len,
                        static_cast<double>(per_wg * word) / 1073741824.0);
        grid = std::min(grid, std::max<long long>(1, static_cast<long long>(budget / (per_wg * word))));
    }
    p.wide_T = T; p.wide_strips = nstrips; p.per_wave = per_wg; p.word_bytes = word; p.grid = grid;
    p.lds = sizeof(double) * p.rows.size() + static_cast<size_t>(T) * (2 * 8 + 2 * 8 + 2 * 4) + static_cast<size_t>(WIDE_CH) * (8 + 8 + 4) +
            WIDE_RING * sizeof(uint16_t);
    if (p.lds > 150 * 1024) return fail("sarlacc_amd: alignment tables do not fit in LDS");
    // global mode, no penalty selects, one strip: the kernel without a barrier per step (k_align_wide_q); align_wide_barrier = 1: the A/B
    p.wide_queue = !p.pensel && !job.local && nstrips == 1 && !option(OPT_ALIGN_WIDE_BARRIER);
    if (!p.wide_queue) return 0;
    const int NWV = T / 64;
    p.lds = sizeof(double) * p.rows.size() + static_cast<size_t>(NWV) * WQ_B * (8 + 8 + 4) + static_cast<size_t>(2 * NWV + 2) * 4 +
            static_cast<size_t>(NWV) * 128 * sizeof(uint16_t);
    if (p.lds > 150 * 1024) return fail("sarlacc_amd: alignment tables do not fit in LDS");
    // With traceback: codes only for the steps that can hold cells within WIDE_BAND rows of the main diagonal (40 % of the steps
    // at 2 kb x 2 kb), then a second launch, with the codes of every cell, over the reads whose walks left them (their count
    // stays on the device: no wait in between; none for reads of the reference's molecule).  align_wide_band = -1: no band.
    p.wide_band = kernel_mode == 0 || option(OPT_ALIGN_WIDE_BAND) < 0 ? 0 : (option(OPT_ALIGN_WIDE_BAND) > 0 ? option(OPT_ALIGN_WIDE_BAND) : WIDE_BAND);
    return 0;
}

// The framed locator's LTRIM (k_align): 1 the jump score's hand-over folded into its max (lane_shr1_max), 2 the staging
// prefetch kept as raw load results until the next refill (RAWPF); both by default.  align_locate_trim = -1: neither (the
// loop as it was: A/B, tests), 1 / 2: that one alone.
static int locate_trim() {
    const int o = option(OPT_ALIGN_LOCATE_TRIM);
    return o < 0 ? 0 : o == 0 ? 3 : (o & 3);
}

// No HIP call and no allocation: the small per-call tables, the shape, the mode and the sizes of tiles, grid and LDS (and,
// for MODE 4, the locator's tables in `lp`).
static int plan_align(const AlignJob& job, int num_cu, AlignPlan& p, LocPlan& lp) {
    const int R = job.R, enc_n = job.sc.enc_n;
    std::vector<double> tab;
    build_tables(job.sc.enc_errors, enc_n, tab);
    p.rowzero.assign(R + 1, 0.0);
    for (int col = 1; col <= R; ++col) p.rowzero[col] = p.rowzero[col - 1] - (col == 1 ? p.GO : p.GE);  // (:115-118)
    std::vector<uint32_t> colinfo(R + 1, 0);
    for (int col = 1; col <= R; ++col)
        if (column_info(job.ref[col - 1], &colinfo[col])) colinfo[col] = 7u | (4u << 8) | (4u << 16);  // caller reports the error
    build_cost_rows(tab, enc_n, colinfo.data(), R, p.rows, p.colbase);
    if (4u * enc_n * sizeof(double) + enc_n * sizeof(double) > 0xffffu) return fail("sarlacc_amd: encoding vector too long for the staged read format");
    const int32_t max_len = job.batch.max_len;
    const bool local = job.local;
    int kernel_mode = job.kernel_mode;
    const bool wide = p.wide = R > MAX_REF;   // one workgroup per alignment instead of (a part of) one wavefront
    // gapopen >= 0 (GO >= GE): no penalty selects on the device, see k_align
    bool pensel = !(p.GO >= p.GE);
    pensel = pensel || option(OPT_ALIGN_PENSEL) != 0;  // testing: force the general path
    Shape sh = wide ? Shape{1, 64, 1, 0} : pick_shape(R);
    // interleaved alignments exist for the local modes without penalty selects (adaptor_align by snapshots, score-only);
    // align_interleave = -1: the A/B without them
    const bool il_mode = local && !pensel && (kernel_mode == 0 || kernel_mode == 1);
    if (sh.rowf == 2 && (!il_mode || option(OPT_ALIGN_INTERLEAVE) < 0)) {
        const int K = R > 16 ? 2 : 1;
        sh = {K, 16, NGMAX, 1};
    }
    if (const int K = option(OPT_ALIGN_K)) {  // tuning override
        const int W = (R + K - 1) / K;
        if ((K == 1 || K == 2 || K == 4 || K == 8 || K == 16) && W <= 64) {
            const int Wp = W <= 16 ? 16 : W;
            sh = {K, Wp, std::min(64 / Wp, NGMAX), Wp == 16 ? 1 : 0};
            if (option(OPT_ALIGN_INTERLEAVE) > 0 && il_mode && W <= 8 && (K == 2 || K == 4)) sh = {K, 8, NGMAX2, 2};
        }
    }
    const long long nitems = (job.batch.n + sh.ngroups - 1) / sh.ngroups;
    // traceback tile of one resident wave: one word per lane per TbSteps<K> steps (4 bits per cell)
    const int tb_steps = std::max(1, 8 / sh.K);
    const size_t word_bytes = sh.K == 16 ? 8 : 4;
    size_t per_wave_elems = kernel_mode ? ((static_cast<size_t>(max_len) + sh.W + 16) / tb_steps + 2) * 64 : 0;
    // adaptor_align without penalty selects: snapshots + windowed recompute instead of the code stream
    if (kernel_mode == 1 && local && !pensel) {
        kernel_mode = 3;
        const size_t nsnap = (static_cast<size_t>(max_len) + sh.W + 16) / SNAP_P + 2;
        per_wave_elems = static_cast<size_t>(snap_win(R, sh.W) / tb_steps) * 64 +
                         nsnap * (2 * sh.K + 3) * 64 * (sizeof(double) / word_bytes);
    }
    // ... and, where eligible, by the integer locator + one fp64 window, the snapshot kernel redoing the reads it
    // cannot certify (same tiles).  align_locate = -1: the snapshot path alone (A/B); 2: the un-framed locator, 3: the same
    // at the frame's k (A/B)
    const int loc_frame = option(OPT_ALIGN_LOCATE) == 2 ? 0 : option(OPT_ALIGN_LOCATE) == 3 ? 2 : 1;
    if (kernel_mode == 3 && sh.rowf == 2 && option(OPT_ALIGN_LOCATE) >= 0 &&
        plan_locate(p.rows, p.colbase, enc_n, R, p.GO, p.GE, p.rowzero, max_len, loc_frame, lp))
        kernel_mode = 4;
    // MODE 4 with window classes (align_window_classes = -1: without, A/B): its own tiles hold the codes of one window and
    // the two small snapshot launches get tiles of their own
    const bool classes = p.classes = kernel_mode == 4 && option(OPT_ALIGN_WINDOW_CLASSES) >= 0;
    // (the locator serves eight-lane alignments only: R <= 32, W = 8, a tile of 120 steps at most)
    if (classes && snap_win(R, sh.W) / 8 >= LOC_NCLS) return fail("sarlacc_amd: internal error: window tile of %d steps exceeds the window classes", snap_win(R, sh.W));
    const size_t redo_per_wave = per_wave_elems;
    if (classes) per_wave_elems = static_cast<size_t>(snap_win(R, sh.W) / tb_steps) * 64;
    // workgroups of NWAVES wavefronts; every wavefront owns a traceback tile
    long long grid = align_grid(nitems, NWAVES, num_cu);
    if (kernel_mode) {
        const size_t budget = static_cast<size_t>(6) << 30;
        const long long fit = std::max<long long>(1, static_cast<long long>(budget / std::max<size_t>(1, per_wave_elems * word_bytes * NWAVES)));
        grid = std::min(grid, fit);
    }
    if (classes) {
        // about one workgroup per four CUs, each wavefront with a whole tile (codes of a window + snapshots)
        const size_t wg_bytes = std::max<size_t>(1, redo_per_wave * word_bytes * NWAVES);
        p.redo_grid = static_cast<int>(std::max<size_t>(1, std::min<size_t>((num_cu + 3) / 4, (static_cast<size_t>(6) << 30) / wg_bytes)));
        p.redo_per_wave = redo_per_wave;
    }
    const size_t lds = sizeof(uint16_t) * NWAVES * (sh.rowf == 2 ? NGMAX2 * (RING + RING_MIRROR) : NGMAX * RING_SLOT) + sizeof(double) * p.rows.size() +
                       sizeof(int32_t) * NWAVES * sh.ngroups * (R + 1) + 16;
    if (!wide && lds > 64 * 1024) return fail("sarlacc_amd: alignment tables do not fit in LDS");
    // MODE 4: the window's codes also in an LDS ring of win_nb blocks per wavefront behind the maps (WIN_LDS_WAVES), as many
    // blocks as the 64 KB leave at most.  align_window_lds = -1: the global tile alone (A/B, tests); >= 2: that many blocks
    // (tests: a small ring wraps often and sends most walks to the tile)
    if (kernel_mode == 4 && option(OPT_ALIGN_WINDOW_LDS) >= 0) {
        int& win_nb = p.win_nb;
        const int tile_blocks = snap_win(R, sh.W) / tb_steps;
        win_nb = option(OPT_ALIGN_WINDOW_LDS) >= 2 ? option(OPT_ALIGN_WINDOW_LDS) : win_ring_blocks(R, sh.W, tb_steps);
        win_nb = std::min(win_nb, tile_blocks);
        const size_t block_bytes = static_cast<size_t>(NWAVES) * 64 * sizeof(uint32_t);
        win_nb = static_cast<int>(std::min<size_t>(win_nb, (64 * 1024 - lds) / block_bytes));
        if (win_nb < 2) win_nb = 0;
    }
    p.sh = sh; p.klast = sh.rowf == 2 || sh.K <= 2 ? (R - 1) % sh.K : -1; p.mode = kernel_mode; p.pensel = pensel;
    p.per_wave = per_wave_elems; p.word_bytes = word_bytes; p.grid = grid; p.lds = lds;
    // The locator hands its results over per read, so it need not share the windows' shape: in the frame, with both trims
    // and 25 to 32 columns it runs eight columns per lane, sixteen alignments per wavefront (ROWF 4), which halves the
    // per-lane work around the recurrence per cell.  align_locate_shape = -1: the windows' shape (A/B, tests).
    p.loc_sh = sh; p.loc_klast = p.klast; p.loc_grid = grid;
    if (kernel_mode == 4 && lp.framed && sh.rowf == 2 && sh.K == 4 && R >= 25 && R <= 32 && locate_trim() == 3 &&
        option(OPT_ALIGN_LOCATE_SHAPE) >= 0) {
        p.loc_sh = {8, 4, NGMAX4, 4};
        p.loc_klast = (R - 1) % 8;
        p.loc_grid = align_grid((job.batch.n + NGMAX4 - 1) / NGMAX4, NWAVES, num_cu);   // (the locator writes no tile)
    }
    return wide ? plan_wide(job, num_cu, p) : 0;
}

// What a MODE 4 call with window classes launches beside its arguments: the window order (k_loc_order's output, [n + 2]),
// the tiles of the two small snapshot launches and the side stream they fork onto
struct LocLaunch { int* order = nullptr; void* redo_dirs = nullptr; hipStream_t side = nullptr; hipEvent_t fork = nullptr, join = nullptr; };

// A per-call table: uploaded by the call's first chunk, still in place for the later chunks of the same call.
template <typename T, typename D>
static int call_table(const ChunkOpts& co, const char* name, const T* host, size_t count, D** dev, hipStream_t s) {   // (D: T or const T)
    return co.init_bad ? upload(name, host, count, const_cast<T**>(dev), s) : scratch(name, count, const_cast<T**>(dev));
}

// Every device pointer of the arguments (the outputs apart, which the caller owns), allocated, uploaded or reset.
static int align_buffers(const AlignJob& job, const AlignPlan& p, const LocPlan& lp, const ChunkOpts& co, AlignArgs& a, LocLaunch& ll) {
    Context& c = ctx();
    hipStream_t stream = job.stream;
    const size_t n = static_cast<size_t>(job.batch.n), nsec = static_cast<size_t>(job.nsec);
    SL_TRY(call_table(co, "align.tab", p.rows.data(), p.rows.size(), &a.tables, stream));
    SL_TRY(call_table(co, "align.rz", p.rowzero.data(), p.rowzero.size(), &a.rowzero, stream));
    SL_TRY(call_table(co, "align.cb", p.colbase.data(), p.colbase.size(), &a.colbase, stream));
    SL_TRY(call_table(co, "align.ref", reinterpret_cast<const uint8_t*>(job.ref), static_cast<size_t>(job.R), &a.refchars, stream));
    if (nsec) {
        SL_TRY(call_table(co, "align.ss", job.sec_starts, nsec, &a.sec_s, stream));
        SL_TRY(call_table(co, "align.se", job.sec_ends, nsec, &a.sec_e, stream));
    }
    static const int sentinel[2] = {std::numeric_limits<int>::max(), 0};   // [0] bad-quality read, [1] walk exceeded its bound
    SL_TRY(call_table(co, "align.bad", sentinel, 2, &a.badqual, stream));
    if (p.mode == 4) {
        static const int zero[LOC_STATS] = {};   // (static, as the sentinel: the copies may outlive this frame)
        SL_TRY(call_table(co, "align.ltab", lp.tab.data(), lp.tab.size(), &a.loc_tab, stream));
        SL_TRY(call_table(co, "align.lrz", lp.rz.data(), lp.rz.size(), &a.loc_rz, stream));
        SL_TRY(call_table(co, "align.lstats", zero, LOC_STATS, &a.loc_stats, stream));
    }
    // a chunk that returns without waiting for its kernel must not leave copies from the caller's
    // vectors in flight (nothing else is queued on the stream yet)
    if (co.init_bad && !co.finish) SL_HIP(hipStreamSynchronize(stream));
    if (p.wide) {
        if (p.per_wave) SL_TRY(c.buffer("align.dirs", static_cast<size_t>(p.grid) * p.per_wave * p.word_bytes, &a.dirs));
        SL_TRY(scratch("align.bnd", p.wide_strips > 1 ? static_cast<size_t>(p.grid) * 6 * (static_cast<size_t>(job.batch.max_len) + 2) : 8, &a.wide_bnd));
        if (p.wide_band > 0) {
            SL_TRY(scratch("align.redo", n + 2, &a.wide_redo));
            SL_HIP(hipMemsetAsync(a.wide_redo, 0, sizeof(int), stream));
        }
        return 0;
    }
    if (p.mode) SL_TRY(c.buffer("align.dirs", static_cast<size_t>(p.grid) * NWAVES * p.per_wave * p.word_bytes, &a.dirs));
    if (p.mode != 4) return 0;
    SL_TRY(scratch("align.lredo", n + 2, &a.loc_redo));
    SL_TRY(scratch("align.lout", n * 3, &a.loc_out));
    SL_HIP(hipMemsetAsync(a.loc_redo, 0, 2 * sizeof(int), stream));
    if (p.classes) {
        SL_TRY(scratch("align.lcls", n, &a.loc_cls));
        SL_TRY(scratch("align.lccount", static_cast<size_t>(2 * LOC_NCLS), &a.loc_ccount));
        SL_TRY(scratch("align.lover", n + 2, &a.loc_over));
        SL_TRY(scratch("align.lorder", n + 2, &ll.order));
        SL_HIP(hipMemsetAsync(a.loc_ccount, 0, 2 * LOC_NCLS * sizeof(int), stream));
        SL_HIP(hipMemsetAsync(a.loc_over, 0, 2 * sizeof(int), stream));
        SL_TRY(c.buffer("align.rdirs", static_cast<size_t>(p.redo_grid) * std::max<size_t>(1, p.redo_per_wave * p.word_bytes * NWAVES), &ll.redo_dirs));
        SL_TRY(c.side_stream(&ll.side, &ll.fork, &ll.join));
    }
    return 0;
}

// ... and everything else in them, from the job and the plan.
static void align_args(const AlignJob& job, const AlignPlan& p, const LocPlan& lp, const ChunkOpts& co, AlignArgs& a) {
    const AlignOut& out = job.out;
    a.seq = job.batch.d_seq; a.nmask = job.batch.d_nmask; a.qual = job.batch.d_qual; a.off = job.batch.d_off; a.n = job.batch.n;
    a.R = job.R; a.W = p.sh.W; a.ngroups = p.sh.ngroups; a.local = job.local ? 1 : 0;
    a.qoffset = static_cast<int>(job.sc.enc_names[0]); a.navail = job.sc.enc_n;
    a.GO = p.GO; a.GE = p.GE;
    a.tab_doubles = static_cast<int>(p.rows.size()); a.row_bytes = static_cast<int>(job.sc.enc_n * sizeof(double));
    a.scores = out.d_scores; a.starts = out.d_starts; a.ends = out.d_ends;
    a.nsec = job.nsec; a.sec_so = out.d_sec_so; a.sec_wo = out.d_sec_wo;
    a.dirs_per_wave = p.per_wave;
    a.read_base = co.read_base; a.sec_stride = co.sec_stride ? co.sec_stride : job.batch.n;
    a.snap_head = snap_head(job.R); a.snap_win = snap_win(job.R, p.sh.W);
    a.aln_ref = out.d_aln_ref; a.aln_qry = out.d_aln_qry; a.aln_len = out.d_aln_len; a.edits = out.d_edits;
    a.win_nb = p.win_nb;
    if (p.wide) { a.wide_maxlen = job.batch.max_len; a.wide_band = p.wide_band; }
    if (p.mode == 4) {
        a.loc_GO = lp.GO; a.loc_GE = lp.GE; a.loc_D = lp.D; a.loc_force = option(OPT_ALIGN_LOCATE) == 1 ? 1 : 0;
        a.loc_framed = lp.framed ? 1 : 0;
        a.loc_unit = lp.unit; a.loc_slack = lp.slack; a.loc_top = lp.top;
    }
}

// Dynamic LDS beyond 48 KB needs the kernel's limit raised first.  The attribute belongs to the function on ONE device: it is
// remembered per (device, kernel), so it is raised once and not at every launch, and once more on this thread's next device.
static int raise_dynamic_lds(const void* kernel, size_t bytes) {
    static thread_local std::map<std::pair<int, const void*>, size_t> limit;
    if (bytes <= 48 * 1024) return 0;
    size_t& set = limit[{ctx().device, kernel}];
    if (bytes > set) SL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    set = std::max(set, bytes);
    return 0;
}

// The instantiations of k_align the library is built with (each costs compile time and code-object size).
// KLAST is known for one or two columns per lane and for interleaved alignments.
constexpr bool shape_exists(int K, int rowf, int klast) {
    if (rowf == 4) return K == 8 && klast >= 0 && klast < K;   // the framed locator of 25 to 32 columns
    if (rowf == 2) return (K == 2 || K == 4) && klast >= 0 && klast < K;
    return K <= 2 ? klast >= 0 && klast < K : klast == -1;
}
constexpr bool mode_exists(int rowf, int mode, bool local, bool pensel, bool wlds, int ltrim) {
    if (ltrim != 0 && mode != 6) return false;
    if (rowf == 4) return local && !pensel && !wlds && mode == 6 && ltrim == 3;   // plan_align asks for nothing else
    // interleaved alignments: local mode without penalty selects only (adaptor_align by snapshots or by the locator 5 / 6 and
    // its window 4, score-only)
    if (rowf == 2) return local && !pensel && (wlds ? mode == 4 : (mode == 0 || (mode >= 3 && mode <= 6)));
    // adaptor_align is always local, general_align always global; score-only comes in both
    return !wlds && (mode == 0 || (mode == 1 && local) || (mode == 3 && local && !pensel) || (mode == 2 && !local));
}

// One launch of k_align in shape `sh`; `mode` and `wlds` are the launch's (MODE 4 is a sequence of several).
// (ltrim: the framed locator's LTRIM, see locate_trim)
static int launch_shape(const Shape& sh, int klast, bool pensel, int mode, bool wlds, const AlignArgs& a, int grid, size_t lds, hipStream_t s,
                        int ltrim) {
    const bool il = sh.rowf == 2 || sh.rowf == 4;
    if (ltrim && mode != 6) return fail("sarlacc_amd: internal error: a trimmed locator outside the frame");
    const int rc = pick([&](auto k_, auto r_, auto l_) {
        constexpr int K = decltype(k_)::value, ROWF = decltype(r_)::value, KLAST = decltype(l_)::value;
        if constexpr (!shape_exists(K, ROWF, KLAST)) return NO_KERNEL;
        else {
            const int rcm = pick([&](auto m_, auto g_, auto p_, auto w_, auto t_) {
                constexpr int MODE = decltype(m_)::value, LTRIM = decltype(t_)::value;
                constexpr bool LOCAL = decltype(g_)::value != 0, PENSEL = decltype(p_)::value != 0, WLDS = decltype(w_)::value != 0;
                if constexpr (!mode_exists(ROWF, MODE, LOCAL, PENSEL, WLDS, LTRIM)) return NO_KERNEL;
                else {
                    if constexpr (WLDS) SL_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&k_align<K, MODE, LOCAL, ROWF, KLAST, PENSEL, WLDS, LTRIM>), lds));
                    hipLaunchKernelGGL((k_align<K, MODE, LOCAL, ROWF, KLAST, PENSEL, WLDS, LTRIM>), dim3(grid), dim3(64 * NWAVES), lds, s, a);
                    return 0;
                }
            }, Ints<0, 1, 2, 3, 4, 5, 6>{}, mode, Ints<0, 1>{}, a.local, Ints<0, 1>{}, pensel, Ints<0, 1>{}, wlds, Ints<0, 1, 2, 3>{}, ltrim);
            return rcm != NO_KERNEL ? rcm : fail(il ? "sarlacc_amd: interleaved alignments serve local modes 0 and 3 only" : "sarlacc_amd: unsupported alignment mode");
        }
    }, Ints<1, 2, 4, 8, 16>{}, sh.K, Ints<0, 1, 2, 4>{}, sh.rowf, Ints<-1, 0, 1, 2, 3, 4, 5, 6, 7>{}, klast);
    // (an interleaved shape with K and mode both unknown raised the mode's message before: plan_align produces neither)
    return rc != NO_KERNEL ? rc : fail(il ? "sarlacc_amd: unsupported columns-per-lane %d for interleaved alignments" : "sarlacc_amd: unsupported columns-per-lane %d", sh.K);
}
// ... in the plan's shape
static int launch_k(const AlignPlan& p, int mode, bool wlds, const AlignArgs& a, int grid, size_t lds, hipStream_t s, int ltrim = 0) {
    return launch_shape(p.sh, p.klast, p.pensel, mode, wlds, a, grid, lds, s, ltrim);
}

// MODE 4: the locator, the windows, the snapshot kernel on what they could not certify.
static int launch_locate(const AlignPlan& p, const AlignArgs& a, const LocLaunch& ll, hipStream_t s) {
    const int grid = static_cast<int>(p.grid);
    // the locator (its LDS: rings + the integer table), the windows, then the snapshot kernel on the reads the windows
    // put on their list (count read on the device)
    const size_t lds5 = sizeof(uint16_t) * NWAVES * p.loc_sh.ngroups * (RING + RING_MIRROR) + sizeof(int) * a.tab_doubles + 16;
    SL_TRY(launch_shape(p.loc_sh, p.loc_klast, p.pensel, a.loc_framed ? 6 : 5, false, a, static_cast<int>(p.loc_grid), lds5, s,
                        a.loc_framed ? locate_trim() : 0));
    AlignArgs r = a;
    r.bad_done = 1;
    // the windows: with the code ring in LDS behind the maps (three wavefronts per SIMD), or the tile alone
    const size_t lds4 = p.lds + static_cast<size_t>(NWAVES) * a.win_nb * 64 * sizeof(uint32_t);
    auto windows = [&](const AlignArgs& w) { return a.win_nb ? launch_k(p, 4, true, w, grid, lds4, s) : launch_k(p, 4, false, w, grid, p.lds, s); };
    if (!p.classes) {
        SL_TRY(windows(a));
        r.read_list = a.loc_redo;
        return launch_k(p, 3, false, r, grid, p.lds, s);
    }
    // The locator has listed the oversize reads: the snapshot kernel aligns them on the side stream while this one
    // orders and runs the windows.  Both snapshot launches are small (their item loop strides) and share tiles: the
    // second, on the reads whose walk stalled, starts after the join.
    r.dirs = ll.redo_dirs;
    r.dirs_per_wave = p.redo_per_wave;
    SL_HIP(hipEventRecord(ll.fork, s));
    SL_HIP(hipStreamWaitEvent(ll.side, ll.fork, 0));
    r.read_list = a.loc_over;
    SL_TRY(launch_k(p, 3, false, r, p.redo_grid, p.lds, ll.side));
    SL_HIP(hipEventRecord(ll.join, ll.side));
    hipLaunchKernelGGL(k_loc_order, dim3(static_cast<unsigned>((a.n + 255) / 256)), dim3(256), 0, s, a.loc_cls, a.n, a.loc_ccount, ll.order);
    AlignArgs w = a;
    w.read_list = ll.order;
    w.bad_done = 1;
    SL_TRY(windows(w));
    SL_HIP(hipStreamWaitEvent(s, ll.join, 0));
    r.read_list = a.loc_redo;
    return launch_k(p, 3, false, r, p.redo_grid, p.lds, s);
}

// References beyond MAX_REF columns (the queue kernel with a band runs twice: then with every cell's codes, over the reads whose walks left it).
static int launch_wide(const AlignPlan& p, AlignArgs a, hipStream_t stream) {
    constexpr int K = WIDE_K;
    const dim3 g(static_cast<unsigned>(p.grid)), b(static_cast<unsigned>(p.wide_T));
    const int mode = p.mode == 3 ? 1 : p.mode;
    auto launch_q = [&]() { return pick([&](auto m_) {
        constexpr int MODE = decltype(m_)::value;
        SL_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&k_align_wide_q<K, MODE>), p.lds));
        hipLaunchKernelGGL((k_align_wide_q<K, MODE>), g, b, p.lds, stream, a);
        return 0;
    }, Ints<0, 1, 2>{}, mode); };
    if (p.wide_queue) {
        SL_TRY(launch_q());
        if (p.wide_band <= 0) return 0;
        a.wide_band = 0; a.wide_list = a.wide_redo + 1;
        return launch_q();
    }
    return pick([&](auto m_, auto p_, auto s_) {
        constexpr int MODE = decltype(m_)::value;
        constexpr bool PENSEL = decltype(p_)::value != 0, STRIPS = decltype(s_)::value != 0;
        SL_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&k_align_wide<K, MODE, PENSEL, STRIPS>), p.lds));
        hipLaunchKernelGGL((k_align_wide<K, MODE, PENSEL, STRIPS>), g, b, p.lds, stream, a);
        return 0;
    }, Ints<0, 1, 2>{}, mode, Ints<0, 1>{}, p.pensel, Ints<0, 1>{}, p.wide_strips > 1);
}

static int report_align(const AlignPlan& p, const LocPlan& lp, const AlignArgs& a, hipStream_t stream, int* bad_qual_read) {
    Context& c = ctx();
    const int *d_stats = a.loc_stats, *d_ccount = a.loc_ccount;
    const bool banded = p.wide && p.wide_queue && p.wide_band > 0;   // (a.wide_redo exists)
    int flags[2] = {0, 0}, lstats[LOC_STATS] = {}, ccount[LOC_NCLS] = {}, wide_redo = 0;
    SL_HIP(hipMemcpyAsync(flags, a.badqual, sizeof flags, hipMemcpyDeviceToHost, stream));
    if (d_stats) SL_HIP(hipMemcpyAsync(lstats, d_stats, sizeof lstats, hipMemcpyDeviceToHost, stream));
    if (d_ccount) SL_HIP(hipMemcpyAsync(ccount, d_ccount, sizeof ccount, hipMemcpyDeviceToHost, stream));
    if (banded) SL_HIP(hipMemcpyAsync(&wide_redo, a.wide_redo, sizeof wide_redo, hipMemcpyDeviceToHost, stream));
    SL_HIP(hipStreamSynchronize(stream));
    *bad_qual_read = flags[0];
    // reads the banded first launch of k_align_wide_q put on its redo list (the second launch adds none), summed over the
    // chunks of a call: run_align's first chunk has set -1, which stands where the banded queue kernel did not run
    if (banded) {
        double& redo = c.counts["align_wide_redo"];
        redo = std::max(redo, 0.0) + wide_redo;
    }
    // adaptor_align calls: reads the locator handed to the snapshot kernel, and walks of its window that stalled (-1: the
    // call ran the snapshot path alone)
    if (p.mode == 3 || p.mode == 4) {
        c.counts["align_redo"] = d_stats ? lstats[0] : -1.0;
        c.counts["align_stalls"] = d_stats ? lstats[1] : -1.0;
        // reads the locator itself listed as oversize (part of align_redo; 0 without window classes), and the steps the
        // window kernel's work items ran (each the tallest of its eight windows)
        c.counts["align_oversize"] = d_stats ? lstats[2] : -1.0;
        unsigned long long wsteps = 0;
        std::memcpy(&wsteps, lstats + 4, sizeof wsteps);
        c.counts["align_window_steps"] = d_stats ? static_cast<double>(wsteps) : -1.0;
        // the code words walks read from the global tile and the walks that read any, the others having stayed in the LDS
        // ring (-1: the call ran without the ring)
        unsigned long long wglob = 0;
        std::memcpy(&wglob, lstats + 6, sizeof wglob);
        c.counts["align_walk_global"] = d_stats && p.win_nb ? static_cast<double>(wglob) : -1.0;
        c.counts["align_walk_left_ring"] = d_stats && p.win_nb ? lstats[3] : -1.0;
        // reads per window class (a class is 8 steps) of the call's last launch, "align_window_class_<c>": diagnostic, for
        // the tests and the perf records
        for (int x = 1; x < LOC_NCLS; ++x) c.counts["align_window_class_" + std::to_string(x)] = d_ccount ? ccount[x] : -1.0;
        // the locator's scale 2^k, negative where it ran un-framed (0: no locator)
        c.counts["align_locate_k"] = d_stats ? (lp.framed ? lp.k : -lp.k) : 0.0;
        // the columns a lane of the locator owns (0: no locator)
        c.counts["align_locate_cols"] = d_stats ? p.loc_sh.K : 0.0;
    }
    if (flags[1]) return fail("sarlacc_amd: internal error: an alignment traceback exceeded its bound");
    return 0;
}

// One reference against a batch on the device: tables, plan, buffers, arguments, launch, report.
// (ChunkOpts, align_host.hpp: a host call may hand its batch over in chunks.)
int run_align(const AlignJob& job, int* bad_qual_read, const ChunkOpts& co) {
    Context& c = ctx();
    hipStream_t stream = job.stream;
    const int64_t n = job.batch.n;
    if (co.init_bad) *bad_qual_read = std::numeric_limits<int>::max();
    if (co.init_bad) c.counts["align_wide_redo"] = -1.0;   // (report_align counts where the banded queue kernel runs)
    if (n <= 0) return 0;
    if (job.sc.enc_n > 256) return fail("sarlacc_amd: encoding vector longer than 256 entries");
    if (n > std::numeric_limits<int>::max() - 8) return fail("sarlacc_amd: more than 2^31 reads in one call");
    AlignPlan p;
    p.GO = job.sc.gapopen + job.sc.gapext; p.GE = job.sc.gapext;  // (src/reference_align.cpp:8)
    if (job.R == 0) {
        const int bs = 256;
        const AlignOut& out = job.out;
        hipLaunchKernelGGL(k_align_emptyref, dim3(static_cast<unsigned>((n + bs - 1) / bs)), dim3(bs), 0, stream,
                           job.batch.d_off, static_cast<long long>(n), job.local ? 1 : 0, p.GO, p.GE, out.d_scores, out.d_starts,
                           out.d_ends, job.nsec, out.d_sec_so, out.d_sec_wo, out.d_aln_len, out.d_edits, job.batch.d_seq,
                           out.d_aln_ref, out.d_aln_qry);
        SL_HIP(hipGetLastError());
        return 0;
    }
    LocPlan lp;
    SL_TRY(plan_align(job, c.num_cu, p, lp));
    AlignArgs a{};
    LocLaunch ll;
    SL_TRY(align_buffers(job, p, lp, co, a, ll));
    align_args(job, p, lp, co, a);
    if (co.stage) SL_TRY(c.stage_begin(co.stage, stream));
    else SL_HIP(hipEventRecord(c.ev_start, stream));
    if (p.wide) SL_TRY(launch_wide(p, a, stream));
    else if (p.mode == 4) SL_TRY(launch_locate(p, a, ll, stream));
    else SL_TRY(launch_k(p, p.mode, false, a, static_cast<int>(p.grid), p.lds, stream));
    SL_HIP(hipGetLastError());
    if (co.stage) {
        SL_TRY(c.stage_end(co.stage, stream));
    } else {
        SL_HIP(hipEventRecord(c.ev_stop, stream));
        c.timed = true;
    }
    return co.finish ? report_align(p, lp, a, stream, bad_qual_read) : 0;
}

}  // namespace sarlacc
