/*
 * sarlacc_amd.h -- C ABI of the MI355X-native sarlacc hot path (libsarlacc_amd.so).
 *
 * Every entry point replaces one `.Call` routine of the reference
 * (/root/reference/src/init.cpp:9-35, prototypes src/sarlacc.h:14-36); the
 * citation next to each declaration names the routine it stands in for.  The
 * reference's SEXP arguments become flat arrays:
 *
 *   XStringSet / character vector  ->  const char* chars (concatenated, no NULs)
 *                                      + const int64_t* off (n+1 offsets)
 *   named numeric `encoding`       ->  const double* enc_errors + const char* enc_names
 *                                      (names[i] is the single-character name of errors[i])
 *   list of integer vectors        ->  CSR: int64 off[n+1] + int32 values (1-based as in R)
 *   numeric / integer scalars      ->  double / int
 *
 * Two levels are exported:
 *   sarlacc_<name>(...)      host pointers in, host pointers out (what a cgo/.Call/ctypes
 *                            shim binds; does the H2D/D2H copies itself);
 *   sarlacc_dev_<name>(...)  device pointers in/out, asynchronous on a caller stream
 *                            (inputs already resident in HBM; used by bench.py and by a
 *                            pipeline that keeps reads on the GPU between stages).
 *
 * All functions return 0 on success.  On failure they return nonzero and
 * sarlacc_last_error() returns the message; messages that the reference throws
 * are reproduced verbatim (src/utils.cpp, src/reference_align.cpp, ...).
 * There is NO CPU fallback: without a usable HIP device every compute entry
 * point fails with an error.
 */
#ifndef SARLACC_AMD_H
#define SARLACC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* library / device management (no reference counterpart)               */
const char* sarlacc_last_error(void);
int sarlacc_version(void);
/* Number of visible HIP devices (0 when none / runtime unavailable). */
int sarlacc_device_count(void);
/* Select the device used by this thread's subsequent calls (default 0). */
int sarlacc_set_device(int device);
/* Release cached device workspaces (and the idle page-locked host blocks of sarlacc_host_alloc). */
void sarlacc_release_workspace(void);
/* Frees only the cached device buffers of the umi_group stage (the neighbour search, the sorted link lists, the clustering:
 * 17 GB after a call on 8 x 10^6 UMIs) -- for pipelines that go on to the MSA stage in the same process and want that memory
 * for it.  Returns the number of bytes given back. */
int64_t sarlacc_release_umi_workspace(void);
/* What the library's cached device buffers hold right now: "name bytes" lines, largest first, into buf (truncated at cap);
 * returns the total in bytes (diagnostics: bench.py reports the largest ones of the giant pre-group leg). */
int64_t sarlacc_workspace_report(char* buf, int64_t cap);
/* Duration in ms of a named group of kernel launches of the last call that ran it (HIP events on
 * the launch stream, summed over the batches of the call): "msa_pairwise", "msa_merge", "consensus", "umi_pairs";
 * <0 if it never ran. */
double sarlacc_stage_ms(const char* name);
/* Work counters of the last call that set them (for rooflines): "msa_pairs", "msa_cells" (banded DP
 * cells of the pairwise alignments), "consensus_cells" (rows x width); "consensus_route" (the kernels the vote ran:
 * 0 k_consensus<false>, 1 k_consensus<true>, 2 k_consensus_q4, 3 k_consensus_qf then k_consensus_q4 on the groups it
 * flagged, 4 k_consensus_code) and "consensus_vote_passes" (1 + the runs repeated for a longer boundary list); of every
 * UMI neighbour search "umi_pairs_words" (64-bit code words per string: 1 up to 32 bases, 4 up to 128, beyond what the
 * longest string needs) and "umi_pairs_k" (the template K of the tile-pair kernel it ran: k_umi_pairs<K> at one word,
 * k_umi_pairs_long<K, XL> beyond; -1 the long kernels' full DP; -2 no tile-pair kernel at all: a split-key search with no
 * string that holds an N or is shorter than 8 bases, or a negative threshold); <0 if unset (-1).  Read
 * "umi_pairs_words" first: while it is > 0 a search has run and an "umi_pairs_k" of -1 is the full DP, not "unset".
 * Of every greedy clustering: "umi_links" (entries of the neighbour lists), "umi_cluster_rounds" (parallel rounds in all) =
 * "umi_cluster_candidate_rounds" (rounds decided on a candidate window) + "umi_cluster_full_rounds" (rounds over every
 * list), and "umi_cluster_widened" / "umi_cluster_narrowed" (candidate rounds after which the window was doubled / halved). */
double sarlacc_stage_count(const char* name);
/* Duration in ms of the DP kernel launches recorded by the last
 * sarlacc_dev_* align call (HIP events on the launch stream; a panel call: the sum over its DP launches); <0 if none. */
double sarlacc_last_kernel_ms(void);
/* Diagnostic, for tests: what the integer locator of this thread's last adaptor-align call reported, {I_max, lo, hi} per
 * read (lo, hi in units of half a row, see align.hip LOC_NEG), 3 n int32 copied to host memory.  Valid until the next
 * alignment call; an error where no locator has run for n reads.  Nothing in the reference corresponds. */
int sarlacc_align_locate_records(int32_t* out, int64_t n);

/* ------------------------------------------------------------------ */
/* quality-weighted read-vs-reference DP                                 */

/* Reference (adaptor / barcode) length, all entry points of this section: up to 1 024 columns an alignment runs
 * inside a wavefront (k_align), beyond that one workgroup holds it (k_align_wide: strips of 8 192 columns for
 * longer references); beyond 2^20 columns a call fails with a message.  The reference itself (src/reference_align.cpp:7-13) has no limit. */

/* replaces .Call adaptor_align  (src/adaptor_align.cpp:11-77)
 * sec_starts 0-based, sec_ends 1-based (as passed by R/adaptorAlign.R:158).
 * Outputs: scores[n], starts[n], ends[n] (1-based, 0/0 when empty),
 *          sec_start_out / sec_width_out [nsec][n] row-major. */
int sarlacc_adaptor_align(const char* seq, const int64_t* seq_off,
                          const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n,
                          double gapopen, double gapext,
                          const char* adaptor, int adaptor_len,
                          const int32_t* sec_starts, const int32_t* sec_ends, int nsec,
                          double* scores, int32_t* starts, int32_t* ends,
                          int32_t* sec_start_out, int32_t* sec_width_out);

/* replaces .Call adaptor_align_score_only  (src/adaptor_align.cpp:79-110) */
int sarlacc_adaptor_align_score_only(const char* seq, const int64_t* seq_off,
                                     const char* qual, const int64_t* qual_off, int64_t n,
                                     const double* enc_errors, const char* enc_names, int enc_n,
                                     double gapopen, double gapext,
                                     const char* adaptor, int adaptor_len, double* scores);

/* replaces .Call barcode_align  (src/barcode_align.cpp:10-44), global mode */
int sarlacc_barcode_align(const char* seq, const int64_t* seq_off,
                          const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n,
                          double gapopen, double gapext,
                          const char* reference, int reference_len, double* scores);

/* replaces .Call general_align  (src/general_align.cpp:10-62), global mode.
 * aln_ref / aln_query receive the gapped strings back to back, aln_off[n+1] the
 * offsets; pass edit_only != 0 (then aln_* may be NULL) for scores + edit distances.
 * aln_cap is the capacity of each string buffer (sum(L)+n*R always suffices). */
int sarlacc_general_align(const char* seq, const int64_t* seq_off,
                          const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n,
                          double gapopen, double gapext,
                          const char* reference, int reference_len, int edit_only,
                          double* scores, int32_t* edits,
                          char* aln_ref, char* aln_query, int64_t* aln_off, int64_t aln_cap);

/* replaces .Call mask_bad_bases  (src/mask_bad_bases.cpp:10-52); out has seq_off[n] bytes */
int sarlacc_mask_bad_bases(const char* seq, const int64_t* seq_off,
                           const char* qual, const int64_t* qual_off, int64_t n,
                           const double* enc_errors, const char* enc_names, int enc_n,
                           double threshold, char* out);

/* Device-resident form of the three score/trace entry points above.
 * d_seq/d_qual/d_off are device pointers (one shared offset array: lengths were
 * validated when the batch was uploaded); stream is a hipStream_t (NULL = default).
 *   mode: 0 = local (adaptor_align*), 1 = global (barcode_align/general_align)
 *   d_starts/d_ends/d_sec_* may be NULL for score-only.
 * max_len = longest read in the batch (host-known). */
int sarlacc_dev_align(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off,
                      int64_t n, int32_t max_len,
                      const double* enc_errors, const char* enc_names, int enc_n,
                      double gapopen, double gapext,
                      const char* reference, int reference_len, int mode,
                      const int32_t* sec_starts, const int32_t* sec_ends, int nsec,
                      double* d_scores, int32_t* d_starts, int32_t* d_ends,
                      int32_t* d_sec_start_out, int32_t* d_sec_width_out,
                      void* stream);

/* Resident read format of the DP kernel: 2-bit packed bases (4 per byte, base i of the
 * concatenated batch in bits 2*(i%4) of byte i/4: A=0 C=1 G=2 T=3) plus one exception bit per
 * base (8 per byte) set where the character is not A/C/G/T (such bases mismatch every A/C/G/T
 * reference column, exactly like the reference's `ref==obs` test, src/reference_align.cpp:188).
 * d_packed needs ceil(total/4)+1 bytes, d_nmask ceil(total/8) bytes. */
int sarlacc_dev_pack_reads(const uint8_t* d_seq, int64_t total, uint8_t* d_packed, uint8_t* d_nmask,
                           void* stream);

/* sarlacc_dev_align on the packed format (offsets still count bases). */
int sarlacc_dev_align_packed(const uint8_t* d_packed, const uint8_t* d_nmask, const uint8_t* d_qual,
                             const int64_t* d_off, int64_t n, int32_t max_len,
                             const double* enc_errors, const char* enc_names, int enc_n,
                             double gapopen, double gapext,
                             const char* reference, int reference_len, int mode,
                             const int32_t* sec_starts, const int32_t* sec_ends, int nsec,
                             double* d_scores, int32_t* d_starts, int32_t* d_ends,
                             int32_t* d_sec_start_out, int32_t* d_sec_width_out,
                             void* stream);

/* A whole barcode panel against one batch: the loop of barcodeAlign (R/barcodeAlign.R:20-37) around .Call barcode_align
 * (src/barcode_align.cpp:10-44), with its reduction done on the device.  barcodes / barcode_off[nbarcodes + 1] hold the
 * panel back to back.  For every read, over the barcodes b = 0, 1, ... in panel order with s its global-mode score:
 *     if (s > score) { next = score; score = s; best = b + 1; } else if (s > next) next = s;
 * from best = 0 (none: R's NA), score = next = -inf; both comparisons are strict, so the first of equal scores wins and a
 * score equal to the best one counts as next best.  The caller's gap is score - next.  all_scores, when not NULL, receives
 * every score as [nbarcodes][n]; each is bit for bit what sarlacc_barcode_align gives for that barcode alone.
 * Barcodes of 1 to 32 columns run fused (k_barcode_panel: one launch per run of consecutive such barcodes, reads staged
 * once); the others -- and all of them under option "align_panel" = -1 -- go through the DP of sarlacc_dev_align one at
 * a time into a score row that is folded on the device.  sarlacc_stage_count "panel_fused_barcodes" /
 * "panel_single_barcodes" / "panel_launches" (DP launches) describe the last call, sarlacc_last_kernel_ms its DP launches.
 * n == 0 writes nothing; nbarcodes == 0 gives best 0 and -inf twice.  A call fails with the message the loop over the
 * barcodes would have raised first (each barcode as in sarlacc_barcode_align, in panel order); the outputs are then
 * unspecified.  The device form waits for the stream before it returns. */
int sarlacc_dev_barcode_panel(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off,
                              int64_t n, int32_t max_len,
                              const double* enc_errors, const char* enc_names, int enc_n,
                              double gapopen, double gapext,
                              const char* barcodes, const int64_t* barcode_off, int nbarcodes,
                              int32_t* d_best, double* d_score, double* d_next, double* d_all_scores,
                              void* stream);
int sarlacc_barcode_panel(const char* seq, const int64_t* seq_off,
                          const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n,
                          double gapopen, double gapext,
                          const char* barcodes, const int64_t* barcode_off, int nbarcodes,
                          int32_t* best, double* score, double* next, double* all_scores);

/* ---- resident batches for the scrambled-control callers ----
 * tuneAlignment (R/tuneAlignment.R:30-72) and getAdaptorThresholds
 * (R/getAdaptorThresholds.R:35-48,105-128) align the same read windows many times; these
 * helpers keep them in HBM: plain device allocation / copies, .get_front_and_back
 * (R/adaptorAlign.R:86-95) and .scramble_input (R/getAdaptorThresholds.R:68-92) on the device. */
int sarlacc_dev_malloc(void** p, int64_t bytes);
int sarlacc_dev_free(void* p);
/* (blocks of 1 MB and more are pooled by size -- powers of two, at most 4 GB idle per device --: a freed block waits for the
 * next request of its size; sarlacc_dev_pool_release, and sarlacc_release_workspace, give the idle ones back) */
int sarlacc_dev_pool_release(void);
int sarlacc_dev_upload(void* d, const void* h, int64_t bytes);
int sarlacc_dev_download(void* h, const void* d, int64_t bytes);
/* Page-locked host blocks for results (no reference counterpart: R hands its own vectors to .Call).  A device -> host copy
 * into such a block is one DMA transfer; into pageable memory it goes through the runtime's staging buffer.  Blocks are
 * pooled by size (powers of two from 1 MB); sarlacc_host_free returns a block to the pool, sarlacc_host_release frees the
 * idle blocks.  Any host pointer of this interface may point into one. */
int sarlacc_host_alloc(void** p, int64_t bytes);
int sarlacc_host_free(void* p);
int sarlacc_host_release(void);
/* which = 0: first min(tol,width) bases; which = 1: reverse complement of the last
 * min(tol,width) bases with reversed qualities.  d_woff: offsets of the windows (n+1). */
int sarlacc_dev_windows(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                        const int64_t* d_woff, int which, uint8_t* d_oseq, uint8_t* d_oqual, void* stream);
/* .resolve_strand and the row selection of .align_AA_internal (R/adaptorAlign.R:112-122, :190-207) on the results of four
 * sarlacc_dev_align calls that are still in HBM: cs / ce = adaptor 1 on the front windows / adaptor 2 on the back windows,
 * rs / re = adaptor 1 on the back / adaptor 2 on the front.  Each is ONE block of n alignments with S sections (S = nsec1 for
 * cs, rs, out1; nsec2 for ce, re, out2): double scores[n] | int32 starts[n] | int32 ends[n] | int32 section starts[max(S,1)][n]
 * | int32 section widths[max(S,1)][n] (the five outputs of sarlacc_dev_align at these offsets).  d_rev[r] = 1 iff
 * max(cs,0) + max(ce,0) < max(rs,0) + max(re,0); out1 row r = rs or cs, out2 row r = re or ce. */
int sarlacc_dev_choose_strand(const void* d_cs, const void* d_ce, const void* d_rs, const void* d_re, int64_t n, int nsec1, int nsec2,
                              void* d_out1, void* d_out2, uint8_t* d_rev, void* stream);
/* Sub-sequences of resident reads, straight to host strings (XVector::subseq in .align_and_extract, R/adaptorAlign.R:160-174):
 * output r = width[r] bases from the 1-based position start[r] of read r of batch A -- or of batch B where from_b[r] != 0
 * (from_b may be NULL; adaptorAlign's strand choice takes, per read, the alignment on the front or on the back window).
 * start / width / from_b are host arrays; out_off (n + 1) and out_chars (out_cap bytes) are filled on the host. */
int sarlacc_dev_subseq(const uint8_t* d_seq_a, const int64_t* d_off_a, const uint8_t* d_seq_b, const int64_t* d_off_b,
                       const uint8_t* from_b, const int32_t* start, const int32_t* width, int64_t n, char* out_chars,
                       int64_t out_cap, int64_t* out_off, void* stream);
/* realizeReads on resident reads (R/realizeReads.R:28-43): output r = read d_idx[r] (0-based),
 * reverse-complemented when d_rev[r] != 0 (qualities reversed), cut to the oriented positions
 * d_tstart[r] .. d_tstart[r] + width - 1 (1-based), widths given by the output offsets d_ooff. */
int sarlacc_dev_realize(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const int64_t* d_idx,
                        const uint8_t* d_rev, const int32_t* d_tstart, int64_t n_out, const int64_t* d_ooff,
                        uint8_t* d_oseq, uint8_t* d_oqual, void* stream);
/* Per-read Fisher-Yates shuffle (bases and qualities together), splitmix64 stream per read. */
int sarlacc_dev_scramble(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                         uint64_t seed, uint8_t* d_oseq, uint8_t* d_oqual, void* stream);

/* replaces .Call unmask_alignment  (src/unmask_alignment.cpp:12-59): every 'N'/'n'
 * of a gapped row becomes the base at the same ungapped position of the original sequence.
 * out has the layout of aln. */
int sarlacc_unmask_alignment(const char* aln, const int64_t* aln_off, int64_t naln,
                             const char* orig, const int64_t* orig_off, int64_t norig, char* out);

/* ---- alignment profiling: variable-length results, two-call protocol -- *count / *nins always
 * receive the full number of entries; the arrays are filled only when their capacity suffices. ---- */

/* replaces .Call find_homopolymers  (src/homopolymer.cpp:87-134): runs of two or more equal bases of every (possibly
 * gapped) sequence: idx (0-based sequence), pos (1-based start in the ungapped sequence), size, base. */
int sarlacc_find_homopolymers(const char* seq, const int64_t* off, int64_t n, int32_t* idx, int32_t* pos, int32_t* size,
                              char* base, int64_t cap, int64_t* count);

/* replaces .Call match_homopolymers  (src/homopolymer.cpp:141-209): per alignment and homopolymer of the reference string
 * the longest run of the same base in the read string that overlaps it: idx (0-based alignment), pos (as above), rlen. */
int sarlacc_match_homopolymers(const char* ref, const int64_t* ref_off, int64_t nref, const char* read, const int64_t* read_off,
                               int64_t nread, int32_t* idx, int32_t* pos, int32_t* rlen, int64_t cap, int64_t* count);

/* replaces .Call find_errors  (src/find_errors.cpp:9-121): per base of the (first alignment's) reference the number of
 * alignments whose read shows A, C, G, T or a deletion there, and one (position of the next reference base, 0-based;
 * length) entry per insertion.  *standard_len = bases of the reference; with cap_bases below it (or the count arrays
 * NULL) nothing else is computed. */
int sarlacc_find_errors(const char* ref, const int64_t* ref_off, int64_t nref, const char* read, const int64_t* read_off,
                        int64_t nread, int64_t* standard_len, char* bases, int32_t* to_a, int32_t* to_c, int32_t* to_g,
                        int32_t* to_t, int32_t* deletions, int64_t cap_bases, int32_t* ins_pos, int32_t* ins_len,
                        int64_t cap_ins, int64_t* nins);

/* The profiling workflow on a resident batch in one call: every read aligned to `reference` as sarlacc_general_align
 * aligns it, and the alignments reduced on the device to what sarlacc_find_errors and sarlacc_match_homopolymers give
 * for general_align's strings (src/general_align.cpp:10-62 -> src/find_errors.cpp:9-121 + src/homopolymer.cpp:141-209;
 * R/errorFinder.R, R/homopolymerMatcher.R) -- as histograms: no alignment string and no per-event list leaves the
 * device (profile_reads.hip: k_profile_pairs reads the aligner's end-first strings where they lie).
 * The call does the work, keeps the results in the library's workspace and reports their sizes: *n_ins distinct
 * (position, length) insertion pairs, *n_hp_runs homopolymers of the reference (maximal stretches of two or more equal
 * characters), *n_hp_obs distinct (run, observed length) pairs.  d_scores / d_edits (device, n entries, may be NULL)
 * receive what sarlacc_general_align reports, bit for bit.  sarlacc_profile_fetch then copies out, for the last
 * profile of the calling thread:
 *   counts[5][R]  alignments showing A, C, G, T, a deletion at each reference position;
 *   ins_*         per pair the 0-based position of the next reference base (R: after the last one), the length and
 *                 the number of alignments (int64) with such an insertion, ascending by (position, length);
 *   run_*         start and end (1-based, inclusive) and base of each homopolymer of the reference;
 *   obs_*         per pair the run (index into run_*), the longest overlapping run of the same base in the read (0:
 *                 none) and its multiplicity, ascending by (run, length); the multiplicities of a run add up to n.
 * A capacity below the reported size makes the fetch fail with a message and copy nothing.
 * The batch runs in chunks of reads so that the aligner's strings (2 x (bases + reads x R) bytes) stay within a fixed
 * budget; option "profile_chunk_reads" forces a chunk size.  sarlacc_stage_ms "profile_align" (DP), "profile_kernel"
 * (k_profile_pairs) and "profile_reduce" (merging the events) and sarlacc_stage_count "profile_chunks" describe the last
 * call.  Errors are the chain's, in its order: what sarlacc_general_align raises, then "unknown character '%c' in
 * alignment string" for the first read character other than A/C/G/T opposite a reference base.  n == 0 (where the
 * chain has no reference to take from its first alignment) gives zero counts, the reference's runs and no pairs;
 * reference_len == 0 gives no counts and every non-empty read as one insertion at position 0.  Limits: those of
 * sarlacc_general_align.  The device form waits for the stream before it returns. */
int sarlacc_dev_profile_reads(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n, int32_t max_len,
                              const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                              const char* reference, int reference_len, double* d_scores, int32_t* d_edits,
                              int64_t* n_ins, int64_t* n_hp_runs, int64_t* n_hp_obs, void* stream);
int sarlacc_profile_fetch(int32_t* counts, int32_t* ins_pos, int32_t* ins_len, int64_t* ins_mult, int64_t cap_ins,
                          int32_t* run_start, int32_t* run_end, char* run_base, int64_t cap_runs,
                          int32_t* obs_run, int32_t* obs_len, int64_t* obs_mult, int64_t cap_obs);
/* The same from host string sets (uploaded as by sarlacc_general_align); scores / edits are host arrays, may be NULL. */
int sarlacc_profile_reads(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t n,
                          const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
                          const char* reference, int reference_len, double* scores, int32_t* edits,
                          int64_t* n_ins, int64_t* n_hp_runs, int64_t* n_hp_obs);

/* FASTQ text already in device memory -> resident read batch.  Replaces the
 * host-side ShortRead::FastqStreamer + .FASTQ2QSDS conversion (R/adaptorAlign.R:26-37,:104-110;
 * R/realizeReads.R:15-26).  4-line records, LF or CRLF, trailing blank lines ignored; sequences
 * are upper-cased, read names are the header lines without the '@'.
 * Step 1 indexes the text and reports the sizes the caller has to allocate; step 2 fills
 * d_seq/d_qual (total_bases bytes each), d_off (n+1), d_names (total_name_bytes, may be NULL
 * together with d_name_off) for the text indexed last on this thread. */
int sarlacc_dev_fastq_index(const uint8_t* d_text, int64_t nbytes, int64_t* n_records, int64_t* total_bases,
                            int64_t* total_name_bytes, void* stream);
/* Chunked streaming (the `number` argument of adaptorAlign, R/adaptorAlign.R:8,:26: FastqStreamer(filepath, n=number)):
 * d_text holds a block of the file that may end inside a record.  Reports how many of its leading
 * complete records (all four lines terminated by a newline), at most max_records, form the next
 * chunk and how many bytes they occupy; the caller indexes exactly those bytes, then continues at
 * d_text + consumed_bytes (appending more of the file when n_records < max_records). */
int sarlacc_dev_fastq_split(const uint8_t* d_text, int64_t nbytes, int64_t max_records, int64_t* n_records,
                            int64_t* consumed_bytes, void* stream);
int sarlacc_dev_fastq_extract(const uint8_t* d_text, uint8_t* d_seq, uint8_t* d_qual, int64_t* d_off,
                              uint8_t* d_names, int64_t* d_name_off, void* stream);

/* Resident read batch -> FASTQ text in device memory: the inverse of sarlacc_dev_fastq_extract (the reference writes
 * realizeReads' output and the consensus reads with writeXStringSet, vignettes/correction.Rmd:271-278, :352).
 * Record i of the text is
 *     '@' name '\n' seq '\n' '+' '\n' qual '\n'        (LF only; name_len + 2 L + 6 bytes)
 * where seq and qual are the bytes d_off[i] .. d_off[i + 1] of d_seq and d_qual, copied as they are (no quality encoding
 * is involved), and name the bytes d_name_off[i] .. d_name_off[i + 1] of d_names.  d_names and d_name_off are passed
 * together or both NULL; without them record i is named READ_<first_index + i>, decimal and unpadded (first_index = 1
 * numbers a batch from READ_1; it is not used otherwise).  A name that holds '\n' or '\r' is refused, since such a file
 * cannot be read back: the error is "record K: read name holds a line break" for the lowest such record, K 1-based.
 * Step 1 fills d_rec_off with the n + 1 offsets of the records in the whole text and reports its size; step 2 writes the
 * bytes d_rec_off[first] .. d_rec_off[first + count] of the whole text to d_text[0 ..], so a caller that plans ranges
 * of whole records needs room for one range at a time.  d_text may have any alignment.  n == 0 and count == 0 succeed
 * without a launch.  Both calls return when the device has finished.
 * Compressed output is sarlacc_dev_bgzf_deflate on the formatted text (below).
 * Out of scope: multi-line FASTQ, a repeated name on the '+' line. */
int sarlacc_dev_fastq_format_size(const int64_t* d_off, int64_t n, const uint8_t* d_names, const int64_t* d_name_off,
                                  int64_t first_index, int64_t* d_rec_off, int64_t* total_bytes, void* stream);
int sarlacc_dev_fastq_format(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names,
                             const int64_t* d_name_off, int64_t first_index, const int64_t* d_rec_off, int64_t first,
                             int64_t count, uint8_t* d_text, void* stream);

/* Resident read batch -> unaligned BAM records in device memory: the inverse of sarlacc_dev_bam_reads_extract, with the
 * two-step contract and the argument order of the FASTQ pair above.  Record i is an unmapped, unpaired alignment record
 * (SAM specification section 4.2) of the L = d_off[i + 1] - d_off[i] bases and qualities of read i:
 *     block_size (int32, not counting itself) | refID -1 | pos -1 | l_read_name | mapq 0 | bin 4680 (reg2bin(-1, 0), as
 *     htslib writes an unplaced read) | n_cigar_op 0 | flag 4 | l_seq L | next_refID -1 | next_pos -1 | tlen 0 |
 *     name NUL | SEQ | QUAL                                  (36 + l_read_name + (L + 1) / 2 + L bytes, no tags)
 * SEQ holds 4-bit codes through "=ACMGRSVTWYHKDBN", high nibble first, the low nibble of an odd last byte 0; QUAL holds
 * byte - 33; L = 0 is a record with l_seq 0.  The name is the read's name up to its first space or tab (what samtools
 * import keeps of a FASTQ name line: a QNAME holds no blanks), '*' where nothing is left; without d_names it is
 * READ_<first_index + i>.  What BAM cannot hold is refused by step 1, before any byte is written, as "record K: <reason>"
 * for the lowest such record, K 1-based, within a record in this order: "read name longer than 254 bytes" (after the
 * cut), "read name holds a byte outside '!'..'~'" (in the kept part), "base cannot be stored in BAM" (any byte that is
 * not one of the 15 upper-case letters ACMGRSVTWYHKDBN: '=', lower case and '-' are not mapped to N, since
 * sarlacc_dev_bam_reads_extract could not give them back), "quality byte outside Phred+33" (outside 33..126), "record
 * larger than 2^31 - 1 bytes".
 * Step 1 fills d_rec_off with the n + 1 offsets of the records in the whole record stream (no header in it), reports its
 * size, and fills d_cuts (may be NULL) with 2 n sorted offsets into the same stream, the SEQ start and the QUAL start of
 * every record: the piece boundaries for sarlacc_dev_bgzf_deflate_cuts.  Step 2 writes the bytes d_rec_off[first] ..
 * d_rec_off[first + count] of the stream to d_out[0 ..], at any alignment of d_out.  n == 0 and count == 0 succeed
 * without a launch.  Both calls return when the device has finished.
 * sarlacc_dev_bam_format_size_aux / _format_aux are the same pair with the reads' tags (below: "tags of a resident
 * batch"), d_aux / d_aux_off, behind QUAL: record i ends with its d_aux_off[i + 1] - d_aux_off[i] aux bytes as they lie
 * and block_size counts them.  d_cuts then gets 3 n sorted offsets, SEQ start, QUAL start and tag start of every record
 * (tag bytes are text-like and get a Huffman table of their own under the deflate's 64-byte piece rule); a read without
 * tags has its tag start at its record's end, and equal neighbouring cuts are harmless to sarlacc_dev_bgzf_deflate_cuts
 * (a piece ends at the FIRST cut at least 64 bytes into it).  Step 1 walks every read's aux area and refuses, within a
 * record after the quality refusal and in front of the size refusal, "malformed tags" (see sarlacc_dev_bam_tags_find)
 * and, in an area that is well-formed, "tag XX appears twice" (the first entry whose tag an earlier one carries).
 * With d_aux == NULL (and d_aux_off == NULL) both calls are the pair above: the same bytes, the same 2 n cuts.
 * Out of scope: aligned records, paired flags, qualities written as the 0xff "missing" marker, @RG header lines for
 * the RG tags written; the header and the BGZF container are the caller's (DeviceReads.to_bam). */
int sarlacc_dev_bam_format_size(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                                const uint8_t* d_names, const int64_t* d_name_off, int64_t first_index,
                                int64_t* d_rec_off, int64_t* d_cuts, int64_t* total_bytes, void* stream);
int sarlacc_dev_bam_format(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names,
                           const int64_t* d_name_off, int64_t first_index, const int64_t* d_rec_off, int64_t first,
                           int64_t count, uint8_t* d_out, void* stream);
int sarlacc_dev_bam_format_size_aux(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
                                    const uint8_t* d_names, const int64_t* d_name_off, int64_t first_index,
                                    const uint8_t* d_aux, const int64_t* d_aux_off, int64_t* d_rec_off, int64_t* d_cuts,
                                    int64_t* total_bytes, void* stream);
int sarlacc_dev_bam_format_aux(const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* d_off, const uint8_t* d_names,
                               const int64_t* d_name_off, int64_t first_index, const uint8_t* d_aux, const int64_t* d_aux_off,
                               const int64_t* d_rec_off, int64_t first, int64_t count, uint8_t* d_out, void* stream);

/* Tags of a resident batch.  A read's tags are the raw aux bytes of its BAM record (SAM specification section 4.2.4):
 * everything behind QUAL up to the record's end, in file order, unparsed.  A batch holds them flat, as names are held:
 * d_aux bytes and n + 1 int64 offsets d_aux_off.  An aux area is a run of entries, tag (two bytes) | type letter | value;
 * it is malformed when fewer than 3 bytes are left in front of its end, a type letter is not one of AcCsSiIfZHB, a
 * fixed value or a B header or payload runs past the end, a B subtype is not one of cCsSiIf, or a Z or H has no NUL in
 * front of the end.  No call reads at or behind a read's aux end, whatever the bytes say.
 * sarlacc_dev_bam_tags_find walks the whole aux area of every read, one wavefront per read, so it is also the
 * validator: "read K: malformed tags" for the lowest such read, K 1-based in the batch.  `tag` is two bytes.  Per read
 * it reports the first entry with that tag (a repeated tag counts once, as htslib's bam_aux_get): d_type its type letter
 * (0: absent), d_val_off / d_val_len where its value starts, counted from the read's aux start, and its bytes (Z / H
 * without the NUL, B with its 5-byte header), d_tag_off / d_tag_len the same for the whole entry; all zero where the tag
 * is absent.  The five arrays (n entries each) may all be NULL: validation only.  *n_present is the number of reads that
 * hold the tag, *string_bytes the bytes of their A / Z / H values (either may be NULL).
 * sarlacc_dev_bam_tags_strings turns the result of a find into a flat string set on the device: d_str_off gets n + 1
 * offsets, d_chars (string_bytes bytes) the A / Z / H values, an empty string where the tag is absent.
 * sarlacc_dev_bam_tags_ints turns it into int64 d_values (types cCsSiI, 0 where absent) and a d_present byte mask.
 * Where a read holds the tag with another type either call fails with "read K: tag XX has type T" (lowest read) --
 * f and B values are not decoded, they are kept and written as they lie.
 * sarlacc_dev_bam_tags_splice is the one edit: output read r (n_out of them, their n_out + 1 offsets d_out_off computed
 * by the caller, who holds every length) is the aux area of read d_src[r] (NULL: r, and n_out == n_src) without its byte
 * span [d_cut_off[r], d_cut_off[r] + d_cut_len[r]) (both NULL: nothing cut), followed, where d_mask[r] (NULL: everywhere),
 * by a new entry `tag` of type `kind`: 'Z' with the string r of the flat set d_col_chars / d_col_off (n_out + 1 offsets)
 * and a NUL, 'i' with the int32 d_col_ints[r], 0 for no entry.  So one kernel takes or permutes reads, drops a tag,
 * appends one, or replaces one (cut + append).  The span is clamped to the read's aux area and a d_src outside
 * [0, n_src) reads as an empty area; bytes of d_out_off's ranges that the three sources do not fill are written as 0.
 * d_out may have any alignment.  The kernel does not look into the values: the caller keeps a Z free of bytes outside
 * ' '..'~'.
 * n == 0 (n_out == 0) succeeds without a launch.  All calls return when the device has finished.
 * Out of scope: decoding f and B, rewriting MM / ML / mv after a trim or a reversal. */
int sarlacc_dev_bam_tags_find(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n, const uint8_t* tag, uint8_t* d_type,
                              int64_t* d_val_off, int64_t* d_val_len, int64_t* d_tag_off, int64_t* d_tag_len,
                              int64_t* n_present, int64_t* string_bytes, void* stream);
int sarlacc_dev_bam_tags_strings(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n, const uint8_t* tag,
                                 const uint8_t* d_type, const int64_t* d_val_off, const int64_t* d_val_len, uint8_t* d_chars,
                                 int64_t* d_str_off, void* stream);
int sarlacc_dev_bam_tags_ints(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n, const uint8_t* tag,
                              const uint8_t* d_type, const int64_t* d_val_off, int64_t* d_values, uint8_t* d_present,
                              void* stream);
int sarlacc_dev_bam_tags_splice(const uint8_t* d_aux, const int64_t* d_aux_off, int64_t n_src, const int64_t* d_src, int64_t n_out,
                                const int64_t* d_cut_off, const int64_t* d_cut_len, const uint8_t* tag, int kind,
                                const uint8_t* d_col_chars, const int64_t* d_col_off, const int32_t* d_col_ints,
                                const uint8_t* d_mask, const int64_t* d_out_off, uint8_t* d_out, void* stream);

/* Pre-groups of a read batch from alignment records (generics.readGroups; csrc/read_groups.hip).  Four calls on data
 * already in device memory, each usable alone; names are flat string sets, bytes plus n + 1 int64 offsets, as a batch
 * holds them.  Limits: n_reads, n_records and n are below 2^31.  Every result is exact and the same from run to run:
 * no value depends on the order in which atomics arrive.  All calls return when the device has finished.
 * sarlacc_dev_names_match joins records to reads by name.  A read's key is its name up to, and not including, its first
 * space or tab (the cut sarlacc_dev_bam_format_size makes); a record's name is compared whole.  d_read_of_record[r]
 * (n_records entries) is the 0-based read whose key equals record r's name byte for byte, -1 where there is none;
 * *n_unmatched (may be NULL) counts the latter.  A hash only finds candidates: equality is always decided by the
 * bytes.  Option names_hash_bits (sarlacc_set_option; 0 = all 64 bits, k = 1 .. 64 keeps k bits of the hash for slot
 * and tag) exists so that tests make every probe walk chains of unequal keys.  No byte outside the two name buffers
 * (d_read_off[n_reads] and d_rec_off[n_records] bytes) is read.  Errors:
 *   read names J and K are the same up to their first space or tab      (1-based; K the lowest read that is not the
 *                                                                        first of its key, J the first read of that key)
 *   read name K / record name K: its offsets do not ascend inside the name buffer
 * n_reads == 0 marks every record unmatched.
 * sarlacc_dev_records_pick chooses one record per read: among the records r with d_read_of_record[r] == i the one of
 * greatest d_width[r], the lowest r among equal widths (d_record_of_read[i], -1: none), and counts them
 * (d_records_per_read[i]); n_reads entries each.  "record K: a read index outside the batch or a negative width".
 * sarlacc_dev_locus_labels labels the reads by overlap of their chosen ranges.  d_ref / d_strand ('-' or anything else)
 * / d_start / d_width are the n_records rows d_record_of_read points into.  The reads with a record are sorted by
 * (reference, strand with '+' first unless ignore_strand, start, read index); a group starts where reference or strand
 * change and where start > (greatest end since the group began) + maxgap, end = start + width - 1 in 64 bits, maxgap in
 * 0 .. 2^31 - 1.  d_label[i] (n_reads entries) counts the groups in that order from 0, -1 for a read without a record;
 * *n_groups (may be NULL) is their number.  "read K: its record lies outside the columns, or has a seqname code outside
 * 0 .. 2^30 - 1 or a negative width".
 * sarlacc_dev_labels_csr splits 1 .. n by label: the distinct non-negative labels ascending are the groups, negative
 * labels are dropped.  d_group_off (room for n + 1 entries) gets *n_groups + 1 offsets into d_members (room for n
 * entries; only the first *n_members are defined), the 1-based indices of every group ascending. */
int sarlacc_dev_names_match(const uint8_t* d_read_names, const int64_t* d_read_off, int64_t n_reads,
                            const uint8_t* d_rec_names, const int64_t* d_rec_off, int64_t n_records,
                            int32_t* d_read_of_record, int64_t* n_unmatched, void* stream);
int sarlacc_dev_records_pick(const int32_t* d_read_of_record, const int32_t* d_width, int64_t n_records, int64_t n_reads,
                             int32_t* d_record_of_read, int32_t* d_records_per_read, void* stream);
int sarlacc_dev_locus_labels(const int32_t* d_ref, const uint8_t* d_strand, const int32_t* d_start, const int32_t* d_width,
                             int64_t n_records, const int32_t* d_record_of_read, int64_t n_reads, int64_t maxgap,
                             int ignore_strand, int32_t* d_label, int64_t* n_groups, void* stream);
int sarlacc_dev_labels_csr(const int32_t* d_label, int64_t n, int64_t* d_group_off, int32_t* d_members, int64_t* n_groups,
                           int64_t* n_members, void* stream);

/* Reference-free pre-groups of a read batch from k-mer sketches (generics.sequenceGroups; csrc/sketch.hip; the rules are
 * DESIGN.md §4.19).  Four calls on data already in device memory, each usable alone; labels go to CSR groups by
 * sarlacc_dev_labels_csr.  Every result is exact and the same from run to run: no value depends on the order in which
 * atomics arrive.  All calls return when the device has finished.
 * sarlacc_dev_sketch_reads: the one-permutation MinHash sketch of every read.  d_seq / d_off are the bases and the n + 1
 * offsets of a batch; A, C, G, T in upper case are bases, every other byte breaks a k-mer.  k in 5 .. 31, buckets a power
 * of two in 16 .. 256.  A k-mer's value is lo | hi << 32 (bit i of lo / hi: the low / high bit of the code of its base i,
 * A 0 C 1 G 2 T 3), with canonical != 0 the smaller of that and the value of its reverse complement; its hash is fmix64 of
 * the value, and a k-mer whose hash is 2^64 - 1 counts as absent.  d_sketch[r * buckets + j] is the smallest hash h of
 * read r with h >> (64 - log2 buckets) == j, 2^64 - 1 where there is none; d_nkmers[r] counts the read's present k-mers.
 * No byte outside [d_off[0], d_off[n]) is read.  "read K: its offsets do not ascend inside the sequence buffer".
 * sarlacc_dev_sketch_links: the non-empty entries (h, read) of d_sketch (n * buckets words, below 2^31) are sorted by h,
 * then by read; every entry is paired with the entries at distance 1 .. window (1 .. 64) behind it that hold the same h;
 * shared(a, b) counts the pairs of reads a < b, and a -- b is a link when shared(a, b) >= min_shared (1 .. buckets).
 * *n_pairs is the number of distinct pairs with shared >= 1, *n_links the number of links (either may be NULL); always
 * the full numbers.  d_links (may be NULL: sizing) gets the first `capacity` links as a << 32 | b in ascending order, so a
 * caller whose capacity was below *n_links calls again.
 * sarlacc_dev_components: the connected components of n vertices under n_links links (a << 32 | b, any order, repeats
 * allowed).  d_nkmers (n entries; may be NULL: every vertex counts) marks with a value <= 0 the vertices that are in no
 * group: they get label -1 and their links are ignored.  d_label[v] numbers the components from 0 in ascending order of
 * their lowest vertex; *n_groups (may be NULL) is their number.  "link K: an end outside 0 .. n - 1".
 * sarlacc_dev_links_verify (optional, between the links and the components; DESIGN §4.19 rule 6a): every link a -- b
 * (a << 32 | b, 0 <= a < b < n, n_links of them) is checked by an alignment of its two reads, of la and lb bytes.  Two bytes
 * match when they are the same upper-case A, C, G or T; every other byte matches nothing, itself included.  D_w is the
 * unit-cost edit distance over the cells |j - i| <= w = bandwidth (0 .. 127) of the matrix, infinite for |la - lb| > w; it
 * is the edit distance whenever that is <= w.  The bound of a pair is t = max_diff_ppm (0 .. 999999) * max(la, lb) div
 * 10^6 in 64-bit integers.  The link passes with strand 0 and dist D_w(a, b) when that is <= t; otherwise, and only with
 * both_strands != 0, with strand 1 and dist D_w(a, rc(b)) when that is <= t (rc reverses b and swaps A with T and C with
 * G); otherwise it fails with dist -1 and strand 0.  d_dist and d_strand (may be NULL) have n_links entries in the order
 * of the links; d_kept (may be NULL; room for n_links entries) gets the passing links in that same order, *n_kept (host;
 * may be NULL) their number.  n_links = 0 launches nothing.  No byte outside the two reads of a link is read.  "link K:
 * its ends are not 0 <= a < b < n", "read K: its offsets do not ascend inside the sequence buffer, or it has 2^31 bases
 * or more": nothing that rests on such a link is launched, and d_kept is not written. */
int sarlacc_dev_sketch_reads(const uint8_t* d_seq, const int64_t* d_off, int64_t n, int k, int buckets, int canonical,
                             uint64_t* d_sketch, int32_t* d_nkmers, void* stream);
int sarlacc_dev_sketch_links(const uint64_t* d_sketch, int64_t n, int buckets, int window, int min_shared, uint64_t* d_links,
                             int64_t capacity, int64_t* n_pairs, int64_t* n_links, void* stream);
int sarlacc_dev_links_verify(const uint8_t* d_seq, const int64_t* d_off, int64_t n, const uint64_t* d_links, int64_t n_links,
                             int bandwidth, int64_t max_diff_ppm, int both_strands, int32_t* d_dist, uint8_t* d_strand,
                             uint64_t* d_kept, int64_t* n_kept, void* stream);
int sarlacc_dev_components(const uint64_t* d_links, int64_t n_links, int64_t n, const int32_t* d_nkmers, int32_t* d_label,
                           int64_t* n_groups, void* stream);

/* Resident reads assigned to references (generics.referenceGroups; csrc/ref_map.hip; the rules are DESIGN.md §4.20, M1 to
 * M6).  Both sides are sketched by sarlacc_dev_sketch_reads with the same k and buckets; two calls on data already in
 * device memory follow, each usable alone; the chosen references go to CSR groups by sarlacc_dev_labels_csr.  Every
 * result is exact and the same from run to run: no value depends on the order in which atomics arrive.  Both calls
 * return when the device has finished.
 * sarlacc_dev_sketch_candidates (rules M2 and M3): d_ref_sketch (n_refs * buckets words) and d_read_sketch (n_reads *
 * buckets words), both below 2^31 words, are sketches as sarlacc_dev_sketch_reads writes them: entry j of a sketch is
 * 2^64 - 1 or a hash h with h >> (64 - log2 buckets) == j ("reference sketch K, bucket J: ..." / "read sketch K, bucket J:
 * the entry is neither empty nor a hash of that bucket", K 1-based).  A hit is (read r, reference f, bucket j) with
 * d_read_sketch[r * buckets + j] == d_ref_sketch[f * buckets + j] != 2^64 - 1; every reference that holds the hash
 * counts, however many there are.  shared(r, f) is the number of such j; *n_hits (host; may be NULL) the number of all hits,
 * which must stay below 2^31.  The candidates of a read are the references with shared >= min_shared (1 .. buckets),
 * ranked by shared descending, then by reference ascending; the first max_candidates (1 .. 16) are kept.  d_cand_ref and
 * d_cand_shared (int32, n_reads * max_candidates each) get row r = the kept candidates of read r in rank order, unused
 * slots -1 / 0; d_ncand[r] their number.  n_refs == 0 leaves every row unused; n_reads == 0 launches nothing.
 * sarlacc_dev_candidates_assign (rules M4 and M5): d_cand_ref / d_cand_shared are such a table (a slot of -1 is unused,
 * wherever it stands; rank = slot).  max_diff_ppm in 0 .. 999999: every used slot is checked as
 * sarlacc_dev_links_verify checks a link, with a = the reference (d_ref_seq, the n_refs + 1 offsets d_ref_off) and b =
 * the read (d_read_seq, d_read_off): same equality, D_w with w = bandwidth (0 .. 127), t = max_diff_ppm * max(la, lb) div
 * 10^6, forward first (strand 0), then, only with both_strands != 0, the read reverse-complemented (strand 1: the read is
 * the reference's reverse strand).  Among the slots that pass, the one of smallest dist is chosen, the lowest slot among
 * equals.  max_diff_ppm < 0: no check; slot 0 is chosen if used, with dist -1 and strand 0, and neither sequence buffer
 * is read.  Per read (n_reads entries): d_reference (-1: none), d_strand, d_dist (-1: none, or unchecked), d_shared (the
 * chosen slot's d_cand_shared, 0: none).  d_cand_dist / d_cand_strand (may be NULL; n_reads * max_candidates) get every
 * slot's result: the distance, -1 where the slot is unused, fails or was not checked, and the strand.  *n_checked (host;
 * may be NULL) counts the used slots handed to the check.  No byte outside a pair's two sequences is read.  "read K:
 * candidate outside 0 .. n_refs - 1", "reference K: ..." / "read K: its offsets do not ascend inside the sequence buffer,
 * or it has 2^31 bases or more" (K 1-based): nothing that rests on such an entry is launched. */
int sarlacc_dev_sketch_candidates(const uint64_t* d_ref_sketch, int64_t n_refs, const uint64_t* d_read_sketch, int64_t n_reads,
                                  int buckets, int min_shared, int max_candidates, int32_t* d_cand_ref, int32_t* d_cand_shared,
                                  int32_t* d_ncand, int64_t* n_hits, void* stream);
int sarlacc_dev_candidates_assign(const uint8_t* d_ref_seq, const int64_t* d_ref_off, int64_t n_refs, const uint8_t* d_read_seq,
                                  const int64_t* d_read_off, int64_t n_reads, const int32_t* d_cand_ref, const int32_t* d_cand_shared,
                                  int max_candidates, int bandwidth, int64_t max_diff_ppm, int both_strands, int32_t* d_reference,
                                  uint8_t* d_strand, int32_t* d_dist, int32_t* d_shared, int32_t* d_cand_dist, uint8_t* d_cand_strand,
                                  int64_t* n_checked, void* stream);

/* SAM alignment records already in device memory -> ranges (sam2ranges, R/sam2ranges.R:8-95).  d_text holds
 * body lines of a SAM file (no header), LF or CRLF, blank lines skipped; first_line is the 1-based file line
 * number of its first line, used in error messages.  The caller reads the header: ref_names / ref_off (n_ref + 1
 * offsets) are the seqinfo names in order, '*' included; a record's seqname code is its RNAME's index there.
 * restricted_mask (n_ref bytes, NULL = no restriction) marks the seqinfo names in `restricted`, extra_names /
 * extra_off (n_extra + 1 offsets) the `restricted` names that are not seqinfo names.  A record is kept when
 * !(FLAG & 4), MAPQ >= minq (if use_minq) and RNAME is in `restricted` (if given).  FLAG and MAPQ of every line,
 * and POS, RNAME and CIGAR of kept lines, are validated; the first bad line is the error.
 * Step 1 reports the number of lines of the text (a last line without a newline counts), of kept records and of
 * their QNAME bytes; step 2 fills, for the text indexed last on this thread, n_kept entries of d_ref, d_start,
 * d_width, d_lclip, d_rclip (int32), d_strand ('+' / '-'), the QNAME bytes into d_names and n_kept + 1 offsets
 * into d_name_off. */
int sarlacc_dev_sam_index(const uint8_t* d_text, int64_t nbytes, int64_t first_line, const char* ref_names,
                          const int64_t* ref_off, int64_t n_ref, const uint8_t* restricted_mask, const char* extra_names,
                          const int64_t* extra_off, int64_t n_extra, int use_minq, int64_t minq, int64_t* n_lines,
                          int64_t* n_kept, int64_t* kept_name_bytes, void* stream);
int sarlacc_dev_sam_extract(const uint8_t* d_text, int32_t* d_ref, int32_t* d_start, int32_t* d_width,
                            uint8_t* d_strand, int32_t* d_lclip, int32_t* d_rclip, uint8_t* d_names,
                            int64_t* d_name_off, void* stream);

/* BGZF input (blocked gzip: SAM specification section 4.1, RFC 1951 / RFC 1952): compressed FASTQ and SAM files are
 * inflated on the device, so that the compressed bytes cross the bus and the text never visits the host.
 * sarlacc_bgzf_scan needs no device.  buf holds nbytes of a file from the start of a block on and may end inside a
 * block.  It walks the gzip member headers (ID 1f 8b, CM 8, FLG with FEXTRA, a 'BC' subfield of length 2 holding
 * BSIZE, found among any other subfields) of at most max_blocks blocks and fills comp_off (block k is the bytes
 * comp_off[k] .. comp_off[k + 1] of buf) and text_off (the running sum of the ISIZE fields), max_blocks + 1 entries
 * each; *n_blocks is the number of complete blocks, *used_bytes what they occupy, *last_is_eof whether the last of
 * them is the 28-byte empty end-of-file block (a file without one is not an error).  Errors, K the 1-based block
 * number counted from first_block: "BGZF block K: not a gzip member", "... no BC subfield" (how a plain gzip file is
 * recognised), "... block size field is inconsistent" (BSIZE + 1 below header + trailer), "... uncompressed size
 * exceeds 65536".  Bytes left over at the end of a file are the caller's error ("file ends inside BGZF block K").
 * sarlacc_dev_bgzf_inflate inflates block k of d_comp, header and trailer as in the file, into
 * d_text[d_text_off[k] .. d_text_off[k + 1]); d_text and every block's output may have any alignment.  All of
 * RFC 1951 is read: stored, fixed and dynamic blocks, any number per BGZF block.  With check_crc the trailer's
 * ISIZE and CRC-32 are held against the output.  The lowest failing block is the error, "BGZF block K: <reason>" with
 * K counted from first_block and reason one of: invalid stored block, invalid code lengths, invalid symbol,
 * distance beyond the start of the block, output exceeds the size field, compressed data ends early, length
 * mismatch, CRC32 mismatch.  Nothing is written outside a block's own range of d_text, whatever the input.
 * n_blocks == 0 succeeds without a launch.  The call returns when the device has finished.
 * sarlacc_dev_copy copies bytes within device memory (ranges that do not overlap, any alignment): the tail of one
 * text buffer to the front of the next.  sarlacc_dev_rfind_byte reports the position of the last byte of d_text equal
 * to value (-1: none): where a block of lines ends.  Both return when the device has finished.
 * Out of scope: random access via .gzi, device inflate of gzip that is not BGZF (the Python layer inflates that on
 * the host).
 * BGZF output: text in device memory is deflated on the device, so that only compressed bytes cross the bus.
 * sarlacc_bgzf_deflate_bound needs no device: *n_blocks = ceil(nbytes / 65280) (block k holds the text bytes
 * k * 65280 .. min((k + 1) * 65280, nbytes): 0xff00 as htslib cuts) and *comp_capacity = 65536 * n_blocks, what d_comp
 * must hold; either pointer may be NULL.  sarlacc_dev_bgzf_deflate writes those n_blocks blocks, complete gzip members
 * with the BC subfield, CRC-32 and ISIZE, side by side into d_comp (no end-of-file block: the caller appends the 28
 * bytes once per file); d_comp_off (n_blocks + 1 entries, may be NULL) gets their offsets and *comp_bytes their total.
 * d_text and d_comp may have any alignment.  The encoder is Huffman-only (literals and end-of-block; every table
 * declares one distance code of length 0).  Per block it takes the smallest, by exact bit count and ties in this
 * order, of (a) one dynamic-Huffman deflate block, (b) one dynamic-Huffman deflate block per piece -- a piece ends
 * behind a '\n' that lies at least 64 bytes into it, or at the block's end, so a short line goes with the next one --
 * and (c) one stored deflate block, hence never more than 31 bytes above the text.  mode 0 considers all three, mode 1
 * (a) and (c), mode 2 (c) alone.  The same text and mode give the same bytes.  nbytes == 0 succeeds without a launch
 * (0 blocks, 0 bytes).  Errors: a negative size, "unknown BGZF deflate mode M", "BGZF output capacity C is below the
 * bound B".  The call returns when the device has finished; sarlacc_last_kernel_ms is the encode kernel.  Workspace:
 * one 65536-byte slot per block, 1.004 * nbytes rounded up to whole slots, and 16 bytes per block of sizes.
 * sarlacc_dev_bgzf_deflate_cuts is the same call for bytes without lines (BAM records), except for where the pieces of
 * (b) end: at the first position d_cuts[j] - cut_origin that lies at least 64 bytes into the piece, or at the block's
 * end; newlines play no part.  d_cuts holds n_cuts offsets sorted ascending (NULL with n_cuts == 0); positions <= 0 or
 * >= nbytes are ignored, and n_cuts == 0 makes mode 0 write the bytes of mode 1.
 * Out of scope: LZ77 matching (about 4 % on long reads against 17 % for the per-line tables), .gzi / .csi
 * indexes, compressing on the host.
 * BAM (SAM specification section 4.2: the same container around binary records) -> ranges.  d_bam holds nbytes of
 * inflated BAM in device memory whose byte 0 is the start of an alignment record: the caller reads the header
 * (magic, text, reference list) and starts every later buffer at the carried tail.  A record is block_size (int32)
 * followed by block_size bytes, at any byte alignment.  sarlacc_dev_bam_index locates every record that lies wholly in
 * the buffer -- exactly: each start is reached from byte 0 through size fields alone -- and reports their number in
 * *n_records and in *used_bytes the offset of the first record that does not (nbytes when none is cut): the carry.
 * first_record is the 1-based number of the buffer's first record among the file's alignment records, used in error
 * messages; at_eof says that no bytes follow.  n_ref is the number of references of the header; a record's seqname
 * code is its refID, or n_ref for refID -1 ('*', last in the seqinfo as on the SAM path).  restricted_mask (n_ref + 1
 * bytes, the last for '*', NULL = no restriction) marks the names in `restricted`.  A record is kept when
 * !(flag & 4), mapq >= minq (if use_minq) and its reference is marked (if a mask is given; a refID outside
 * [-1, n_ref) is not).  Errors are "BAM record K: <reason>" for the lowest failing record: "file ends inside the
 * record" (at_eof only), "block size below 32" (negative sizes included), on every record "record fields do not fit
 * its block size" (l_read_name 0, a name without its NUL, l_seq < 0, or name + CIGAR + SEQ + QUAL beyond block_size),
 * and on kept records, in this order: "POS is not a 32-bit integer" (pos 2^31 - 1), "reference ID outside the
 * header's reference list", "no CIGAR on a kept record", "CIGAR operation code above 8", "malformed tags or CG tag
 * behind a long-CIGAR stand-in", "CIGAR length above 2^31 - 1" (the width or a clip), "CIGAR has only H and S
 * operations", "alignment end outside the 32-bit integer range".  A kept record whose CIGAR is <l_seq>S<n>N stands in
 * for one of more than 65 535 operations: its tags are walked, and a CG tag of type B,I with at least one entry is the
 * CIGAR; without a CG tag the two operations stand as they are.
 * sarlacc_dev_bam_extract is step 2 of the same two-step contract as the SAM pair, with the parameters and the
 * thread-local state of sarlacc_dev_sam_extract: start is pos + 1, the names are the read names without their NUL.
 * sarlacc_bam_tile_bytes is the tile of the locator (tests place records around its multiples).  The locator takes
 * 4 bytes of workspace per byte of d_bam.
 * BAM -> resident read batch: SEQ and QUAL of the records, unpacked on the device into the flat layout of
 * sarlacc_dev_fastq_extract.  d_bam, nbytes, first_record, at_eof, *n_records and *used_bytes are those of
 * sarlacc_dev_bam_index, and the records are located the same way.  A record becomes a read unless
 * flag & exclude_flags (0x900 drops secondary and supplementary records, whose reads would appear several times, partly
 * hard-clipped; unmapped records, flag 0x4, are reads); reads keep file order and *n_reads is their number.  SEQ is
 * decoded through "=ACMGRSVTWYHKDBN", high nibble first; QUAL values q in 0..93 become q + 33 (Phred+33).  With
 * flag & 0x10 the stored SEQ is the reverse complement of what was sequenced and the read is restored: bases reversed,
 * each code complemented (its four bits in reverse order: A 1 <-> T 8, C 2 <-> G 4, M 3 <-> K 12, ..., N 15 <-> N), QUAL
 * reversed.  A first QUAL byte of 0xff says the record holds no qualities (section 4.2.3): every quality of the read is
 * then missing_qual + 33, missing_qual in 0..93.  The name is the read name without its NUL (no /1 or /2 is added),
 * l_seq 0 is a read of length 0, tags are left to the _aux_ pair below.  Errors are "BAM record K: <reason>" for the
 * lowest failing record, within a record in this order: the locator's two messages and, on every record, "record fields
 * do not fit its block size" as above; on records that become reads "SEQ holds '='" (a code 0) and "quality value above
 * 93" (0xff anywhere but first included).  All of them are reported by sarlacc_dev_bam_reads_index, which keeps its
 * state thread-local like the pairs above (a later locator run on the thread, sarlacc_dev_bam_index included, ends it).
 * sarlacc_dev_bam_reads_range reports what the reads first .. first + count of the buffer indexed last need: their
 * bases, their name bytes, and in *next_byte the offset of the record behind the last of them (used_bytes for
 * first + count == n_reads, which takes the dropped records at the end along; 0 for first + count == 0): where the carry of
 * a chunk that continues in the next buffer starts.  sarlacc_dev_bam_reads_records reports how many records lie in
 * front of that offset for the reads 0 .. reads_taken: what the next buffer's first_record moves on by.
 * sarlacc_dev_bam_reads_extract fills exactly that range: total_bases bytes of d_seq and of d_qual, count + 1 offsets
 * in d_off that start at 0, the names and count + 1 offsets in d_names / d_name_off (both NULL: no names).  Every
 * output may have any alignment; nothing outside those ranges is written.  count == 0 and nbytes == 0 succeed without a
 * launch.  The three calls return when the device has finished.
 * sarlacc_dev_bam_reads_aux_range / _aux_extract are the same two steps for the reads' tags ("tags of a resident batch"
 * above), over the buffer indexed last: the same thread-local state, ended by the same events.  _aux_range reports the
 * aux bytes of the reads first .. first + count; _aux_extract copies each read's aux area as it lies into d_aux and fills
 * count + 1 offsets in d_aux_off that start at 0.  A record with flag 0x10 has its SEQ and QUAL restored by
 * sarlacc_dev_bam_reads_extract, but its tags are copied unchanged: MM / ML / mv of such a record describe the STORED
 * strand.  The tags are sized on the first of these calls after an index, so a buffer read without them pays nothing;
 * they are not validated here (sarlacc_dev_bam_tags_find is the validator).
 * Out of scope: .bai / .csi random access, CRAM. */
int sarlacc_bgzf_scan(const uint8_t* buf, int64_t nbytes, int64_t max_blocks, int64_t first_block, int64_t* comp_off,
                      int64_t* text_off, int64_t* n_blocks, int64_t* used_bytes, int* last_is_eof);
int sarlacc_dev_bgzf_inflate(const uint8_t* d_comp, const int64_t* d_comp_off, const int64_t* d_text_off, int64_t n_blocks,
                             int64_t first_block, uint8_t* d_text, int check_crc, void* stream);
int sarlacc_bgzf_deflate_bound(int64_t nbytes, int64_t* n_blocks, int64_t* comp_capacity);
int sarlacc_dev_bgzf_deflate(const uint8_t* d_text, int64_t nbytes, int mode, uint8_t* d_comp, int64_t comp_capacity,
                             int64_t* d_comp_off, int64_t* comp_bytes, void* stream);
int sarlacc_dev_bgzf_deflate_cuts(const uint8_t* d_text, int64_t nbytes, const int64_t* d_cuts, int64_t n_cuts,
                                  int64_t cut_origin, int mode, uint8_t* d_comp, int64_t comp_capacity,
                                  int64_t* d_comp_off, int64_t* comp_bytes, void* stream);
int sarlacc_dev_copy(void* d_dst, const void* d_src, int64_t bytes, void* stream);
int sarlacc_dev_rfind_byte(const uint8_t* d_text, int64_t nbytes, int value, int64_t* pos, void* stream);
int sarlacc_dev_bam_index(const uint8_t* d_bam, int64_t nbytes, int64_t first_record, int at_eof, int64_t n_ref,
                          const uint8_t* restricted_mask, int use_minq, int64_t minq, int64_t* n_records,
                          int64_t* used_bytes, int64_t* n_kept, int64_t* kept_name_bytes, void* stream);
int sarlacc_dev_bam_extract(const uint8_t* d_bam, int32_t* d_ref, int32_t* d_start, int32_t* d_width,
                            uint8_t* d_strand, int32_t* d_lclip, int32_t* d_rclip, uint8_t* d_names,
                            int64_t* d_name_off, void* stream);
int sarlacc_bam_tile_bytes(void);
int sarlacc_dev_bam_reads_index(const uint8_t* d_bam, int64_t nbytes, int64_t first_record, int at_eof, int exclude_flags,
                                int64_t* n_records, int64_t* used_bytes, int64_t* n_reads, void* stream);
int sarlacc_dev_bam_reads_range(int64_t first, int64_t count, int64_t* total_bases, int64_t* total_name_bytes,
                                int64_t* next_byte);
int sarlacc_dev_bam_reads_records(int64_t reads_taken, int64_t* n_records);
int sarlacc_dev_bam_reads_extract(const uint8_t* d_bam, int64_t first, int64_t count, int missing_qual, uint8_t* d_seq,
                                  uint8_t* d_qual, int64_t* d_off, uint8_t* d_names, int64_t* d_name_off, void* stream);
int sarlacc_dev_bam_reads_aux_range(int64_t first, int64_t count, int64_t* aux_bytes);
int sarlacc_dev_bam_reads_aux_extract(const uint8_t* d_bam, int64_t first, int64_t count, uint8_t* d_aux, int64_t* d_aux_off,
                                      void* stream);

/* ------------------------------------------------------------------ */
/* masked Levenshtein, neighbour search, clustering                      */

/* replaces .Call compute_lev_masked  (src/compute_lev_masked.cpp:13-64);
 * out has n(n-1)/2 doubles, i-major lower triangle (R 'dist' order). */
int sarlacc_compute_lev_masked(const char* seq, const int64_t* off, int64_t n, double* out);

/* replaces .Call fast_levdist_test  (src/sorted_trie.cpp:304-337).
 * Neighbour lists (1-based) in the reference's trie order.  Two-call protocol:
 * nbr==NULL returns the required size in *nbr_need and fills nbr_off. */
int sarlacc_fast_levdist_test(const char* seq, const int64_t* off, int64_t n, int limit,
                              int64_t* nbr_off, int32_t* nbr, int64_t nbr_cap, int64_t* nbr_need);

/* replaces .Call cluster_umis_test  (src/cluster_umis_test.cpp:8-30).
 * links: CSR of 1-based neighbour lists; clusters returned as CSR of 1-based ids
 * (clu_off needs n+1 entries, clu n entries).  Beyond the reference's own two errors, lists that are not symmetric, miss
 * their own read or name a read twice are refused with a message that names the lowest such list. */
int sarlacc_cluster_umis_test(const int64_t* link_off, const int32_t* links, int64_t n,
                              int64_t* nclusters, int64_t* clu_off, int32_t* clu);

/* replaces .Call umi_group  (src/umi_group.cpp:14-116) followed by the
 * unlist(out, recursive=FALSE) of R/umiGroup.R:22.
 * umi2 may be NULL.  pregroups: CSR of 1-based read ids.  Output clusters as CSR
 * of 1-based read ids (clu_off: total+1 entries, clu: total entries, where
 * total = grp_off[ngroups]). */
int sarlacc_umi_group(const char* umi1, const int64_t* off1,
                      const char* umi2, const int64_t* off2, int64_t n,
                      int thresh1, int thresh2,
                      const int64_t* grp_off, const int32_t* grp, int64_t ngroups,
                      int64_t* nclusters, int64_t* clu_off, int32_t* clu);

/* One giant pre-group across several GPUs: the row tiles of the all-pairs
 * matrix shard; every shard returns its neighbour pairs (rank_i << 32 | rank_j, i < j, ranks in the
 * trie order of the whole set, which every shard computes identically), the pair lists are
 * exchanged (all-gather) and the clustering of umi_group runs on their concatenation.
 * Two-call sizing protocol for `pairs` as in sarlacc_fast_levdist_test. */
int sarlacc_umi_pairs_shard(const char* umi, const int64_t* off, int64_t n, int limit,
                            int shard_index, int shard_count,
                            uint64_t* pairs, int64_t cap, int64_t* npairs);
int sarlacc_umi_group_from_pairs(const char* umi, const int64_t* off, int64_t n, int limit,
                                 const uint64_t* pairs, int64_t npairs,
                                 int64_t* nclusters, int64_t* clu_off, int32_t* clu);

/* The same exchange with the pairs kept in HBM (at 8 x 10^6 reads the lists hold 10^8 pairs; nothing of them crosses
 * PCIe): sarlacc_dev_umi_pairs_shard searches the shard's row tiles and leaves its pairs in the library's workspace on the
 * device, reporting their number; sarlacc_dev_umi_pairs_fetch copies them (device to device) into a caller buffer of at
 * least that many entries -- e.g. the send buffer of an RCCL all-gather -- and must be the next library call of the thread;
 * sarlacc_dev_umi_group_from_pairs clusters from a DEVICE array of pairs (validated on the device; the call waits for the
 * device first, so a collective on another stream has finished writing them).
 * Limits shared by every umi_group entry point: strings of at most 1024 bases (longer ones only alone in their pre-group),
 * characters ACGTN only, and at most 2^32 - 1 neighbour links (self links included) per call -- the lists are explicit as in
 * src/umi_group.cpp:59-103; a threshold that joins most of a large set must be lowered or the reads split into pre-groups. */
int sarlacc_dev_umi_pairs_shard(const char* umi, const int64_t* off, int64_t n, int limit,
                                int shard_index, int shard_count, int64_t* npairs);
int sarlacc_dev_umi_pairs_fetch(uint64_t* d_pairs, int64_t cap);
int sarlacc_dev_umi_group_from_pairs(const char* umi, const int64_t* off, int64_t n, int limit,
                                     const uint64_t* d_pairs, int64_t npairs,
                                     int64_t* nclusters, int64_t* clu_off, int32_t* clu);

/* ------------------------------------------------------------------ */
/* per-group MSA and consensus                                           */

/* Which written specification the MSA stage follows (the reference delegates to SeqAn's
 * T-Coffee, which cannot be run or pinned here): 2 (default) = consistency-based progressive alignment --
 * all-pairs banded alignments, primary library, triplet extension into a bounded library (the direct partner and three
 * further positions per pair and base), neighbour-joining guide tree, progressive
 * heaviest-common-subsequence merging -- for groups of up to 64 reads, 1 = centre-star (also used by spec 2 for
 * larger groups, for reads beyond 65 471 bases and for alignments wider than 65 535 columns).  0 restores the default, spec 2 (SARLACC_MSA_SPEC only sets the
 * value the process starts with: the environment is read once). */
int sarlacc_set_msa_spec(int spec);

/* A/B switches of the tests and the perf tools (every default, 0, is the product path; the table is kOptNames in
 * csrc/common.cpp, the meanings are at enum Opt in csrc/common.hpp and in INTEGRATION.md "Options"):
 *   "msa_spec" (1 / 2), "msa2_general_rows", "msa2_chain_hbm", "msa2_waves_per_cu" (a count), "msa2_single_wave",
 *   "msa2_batches" (a count), "msa2_tight_profiles", "align_pensel", "align_chunks" (a count), "align_k" (columns per lane),
 *   "align_waves_per_cu" (a count), "align_interleave" (-1 never / 1 with align_k), "consensus_chars", "consensus_generic",
 *   "msa_int32", "msa_affine", "msa_bitvector" (-1 never, 2 one kernel for fill and walk), "msa_bitvector_core" (-1 whole
 *   records, 1 one word), "msa_bitvector_tile_gb" (GB), "umi_full_rounds", "umi_tile_search", "umi_split_min" (a set size),
 *   "umi_scan_single", "align_wide_barrier" (references beyond 1 024 columns: the kernel with a barrier per step everywhere),
 *   "align_wide_band" (rows either side of the main diagonal whose cells carry traceback codes in k_align_wide_q's first launch; -1: all;
 *   sarlacc_stage_count "align_wide_redo" reports the last alignment call: the reads that first launch put on its redo list, their
 *   walks having left those cells, summed over the call's chunks; -1 where the banded queue kernel did not run -- scores only,
 *   "align_wide_band" = -1, "align_wide_barrier" = 1, local mode, gapopen < 0, several strips, a reference of up to 1 024 columns),
 *   "msa2_budget_gb" (GB a batch of groups may take), "msa2_max_columns" (a lower ceiling of spec v2's profiles),
 *   "msa2_simple_extend" (the extended library by the one-position-per-lane kernel everywhere), "msa2_wide_extend" (largest
 *   group size of the four-positions-per-lane kernel), "align_locate" (adaptor_align: -1 the snapshot path alone, 1 every read
 *   through the locator's redo list, 2 the locator outside its extension-free frame, 3 the same at the frame's scale;
 *   sarlacc_stage_count "align_redo" / "align_stalls" / "align_locate_k" (the locator's scale 2^k, negative outside the
 *   frame, 0 without a locator) report the last such call, and so do "align_oversize" (the reads of align_redo that the
 *   locator itself listed, their window being taller than the code tile), "align_window_steps" (steps summed over the window
 *   kernel's work items, each the tallest of its eight windows) and "align_window_class_<c>" (reads whose window takes
 *   8 c steps at most, c = 1 .. 31, of the call's last launch)),
 *   "align_window_classes" (adaptor_align by the locator: -1 the windows in index order, one redo list filled by the window
 *   kernel and its launch on the caller's stream instead of the locator's classes, its oversize list and the side stream),
 *   "align_window_lds" (adaptor_align by the locator: -1 the window's traceback codes in the global tile alone, the kernel
 *   at five wavefronts per SIMD; >= 2 that many blocks in the per-wave LDS code ring instead of the default; the counters
 *   "align_walk_global" (code words walks read from the global tile) and "align_walk_left_ring" (walks that read any)
 *   report the last call, -1 without the ring),
 *   "align_locate_trim" (adaptor_align's locator in its frame: -1 the fill loop without its trims; 1 the jump score's lane
 *   hand-over folded into its max alone, 2 the staging prefetch held as raw load results until the next refill alone, 3 both,
 *   which is the default),
 *   "align_locate_shape" (adaptor_align's locator in its frame: 0 eight columns per lane and sixteen alignments per
 *   wavefront for adaptors of 25 to 32 columns, with both trims; -1 the window kernel's shape, four columns per lane and
 *   eight alignments per wavefront, everywhere; sarlacc_stage_count "align_locate_cols" reports the columns per lane of the
 *   last call's locator, 0 without one),
 *   "align_panel" (sarlacc_*barcode_panel: -1 every barcode on its own with the device fold, none by the fused kernel),
 *   "profile_chunk_reads" (sarlacc_*profile_reads: reads per chunk; 0 = as many as the byte budget takes),
 *   "names_hash_bits" (sarlacc_dev_names_match: bits of the name hash kept for slot and tag, 1 .. 64; 0 = all 64.  A test
 *   keeps 1, 2 or 8 so that every probe walks long chains of colliding, unequal keys; the results do not change).
 * The environment (SARLACC_<NAME>) is read once, when the first option is asked for; afterwards only this call changes a
 * value.  Nothing in the reference corresponds. */
int sarlacc_set_option(const char* name, int value);

/* replaces .Call quick_msa  (src/quick_msa.cpp:15-80); argument order as there
 * (the R caller passes -gapOpening as gap_extension and -gapExtension as
 * gap_opening, R/multiReadAlign.R:47).  Groups: CSR of 1-based read ids.
 * Output: for group g, rows_g = size(g) strings of equal width width_out[g],
 * written row-major at out + out_off[g]; out_off has ngroups+1 entries.
 * Two-call protocol: out==NULL fills width_out/out_off only.
 * Scoring domain (also of sarlacc_msa_consensus and sarlacc_dev_msa_consensus; DESIGN.md
 * section 5): the four scores are truncated toward zero to integers, and with S the largest
 * magnitude among them and L the longest read that is a member of a group of the call,
 *     S * (2 L + 2) < 2^27
 * must hold -- otherwise the call fails ("sarlacc_amd: MSA scores outside the scoring domain
 * ...", NaN and infinite scores included) before anything runs.  Inside the domain every
 * pairwise score is exact in 32 bits and far from the kernels' "outside the band" value.
 * Under MSA spec 2 a group whose weights max(match, mismatch, 1) do not fit the 16-bit
 * library records or the 32-bit row and chain sums (group size n, longest read L,
 * P = floor(n/2) ceil(n/2): (n-1) W <= 65535, P (n-1) W < 2^30, P (n-1) W L < 2^32) is aligned
 * by spec 1 instead; sarlacc_stage_count("msa_v1_fallback_weights") counts them (never with
 * match <= 1 and mismatch <= 1).  Which pairwise kernel took the pairs of the last call:
 * sarlacc_stage_count("msa_pairs_bitvector" | "msa_pairs_packed" | "msa_pairs_int32"). */
int sarlacc_quick_msa(const int64_t* grp_off, const int32_t* grp, int64_t ngroups,
                      const char* seq, const int64_t* seq_off, int64_t nseq,
                      double match, double mismatch, double gap_extension, double gap_opening,
                      int bandwidth,
                      int32_t* width_out, int64_t* out_off, char* out, int64_t out_cap);

/* replaces .Call create_consensus_basic_loop  (src/create_consensus.cpp:150-170)
 * and, with ngroups==1 and lerr!=NULL, create_consensus_basic (:137-148).
 * Alignments: aln_off[nrows_total+1] string offsets, grp_rows[ngroups+1] row
 * ranges per alignment.  cons/phred: concatenated outputs with cons_off[ngroups+1];
 * capacity of each is the total alignment width.  lerr (optional) gets the
 * natural-log error of every kept column, same offsets. */
int sarlacc_create_consensus_basic_loop(const char* aln, const int64_t* aln_off,
                                        const int64_t* grp_rows, int64_t ngroups,
                                        double min_cov, double pseudo_count,
                                        char* cons, char* phred, int64_t* cons_off, double* lerr);

/* replaces .Call create_consensus_quality_loop  (src/create_consensus.cpp:287-308)
 * and create_consensus_quality (:274-285).  qual strings are per alignment row,
 * ungapped (consumed positionally, N included). */
int sarlacc_create_consensus_quality_loop(const char* aln, const int64_t* aln_off,
                                          const int64_t* grp_rows, int64_t ngroups,
                                          const char* qual, const int64_t* qual_off,
                                          const int64_t* qgrp_rows,
                                          double min_cov,
                                          const double* enc_errors, const char* enc_names, int enc_n,
                                          char* cons, char* phred, int64_t* cons_off, double* lerr);

/* multiReadAlign + consensusReadSeq in one call (R/multiReadAlign.R:16-47 followed by
 * R/consensusReadSeq.R:14-21; i.e. .Call quick_msa then .Call create_consensus_*_loop): the
 * gapped rows never leave HBM and the quality strings stay in read order (rows find theirs
 * through the group lists), so nothing is re-marshalled between the two stages.  Results are
 * those of sarlacc_quick_msa + sarlacc_create_consensus_{quality,basic}_loop on the same input.
 * qual == NULL selects the basic vote (pseudo_count used), otherwise the quality-weighted vote.
 * cons/phred need the KEPT columns of every group (at most the alignment's width; the exact total is reported in the error
 * message when cons_cap is too small -- the vote has run by then; 1.5 x the longest member per group is a safe first guess:
 * same-molecule groups keep about one read length, and a cluster of several molecules, whose alignment is several reads
 * wide, keeps the columns its majority covers). */
int sarlacc_msa_consensus(const int64_t* grp_off, const int32_t* grp, int64_t ngroups,
                          const char* seq, const int64_t* seq_off,
                          const char* qual, const int64_t* qual_off, int64_t nseq,
                          double match, double mismatch, double gap_extension, double gap_opening,
                          int bandwidth, double min_cov, double pseudo_count,
                          const double* enc_errors, const char* enc_names, int enc_n,
                          char* cons, char* phred, int64_t* cons_off, int64_t cons_cap);

/* sarlacc_msa_consensus with the reads (and, for the quality vote, their quality strings) already
 * resident in HBM, e.g. left there by sarlacc_dev_fastq_extract / sarlacc_dev_realize: d_seq and
 * d_qual are device pointers to the concatenated strings, `off` the HOST copy of their n+1 offsets
 * (byte 0 of d_seq is off[0]; the job list is built from the lengths on the host).  d_qual == NULL
 * selects the basic vote.  Group lists and outputs are host arrays as in sarlacc_msa_consensus. */
int sarlacc_dev_msa_consensus(const int64_t* grp_off, const int32_t* grp, int64_t ngroups,
                              const uint8_t* d_seq, const uint8_t* d_qual, const int64_t* off, int64_t nseq,
                              double match, double mismatch, double gap_extension, double gap_opening,
                              int bandwidth, double min_cov, double pseudo_count,
                              const double* enc_errors, const char* enc_names, int enc_n,
                              char* cons, char* phred, int64_t* cons_off, int64_t cons_cap);

#ifdef __cplusplus
}
#endif
#endif
