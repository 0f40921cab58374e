// readers_host.cpp -- the host side of the four readers (readers.hpp): FASTQ text -> reads, SAM text -> ranges, BAM ->
// ranges, BAM -> reads.  How any input format becomes device arrays is read here, top to bottom:
//
//   the shared pieces   offsets_of (lengths -> offsets), FirstBad (the slot a bad record is reported through), the line
//                       index of text (line_counts, line_starts), the ranges back end of SAM and BAM (ranges_index),
//                       the BAM locator's launch sequence (bam_locate)
//   the index states    what an index call leaves on its thread for the extract steps: the indexed buffer, the counts,
//                       and the device arrays those steps read -- as pointers taken at index time.  live() asks the
//                       Context whether each is still the workspace of its name, so a step that comes after
//                       sarlacc_release_workspace, a change of device or a later index is refused on the host with the
//                       step's missing-index message; no kernel ever reads a freed or a fresh buffer.
//   the entry points    fourteen, in the order of include/sarlacc_amd.h
//
// The kernels and the steps that launch them are in text_lines.hip, fastq.hip, sam.hip, bam.hip and bam_reads.hip.
#include "bam_rec.hpp"
#include "devprim.hpp"
#include "readers.hpp"
#include "text_lines.hpp"

#include "../../include/sarlacc_amd.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace sarlacc {
namespace {

// ---- the shared pieces ----------------------------------------------------------------------------------------------------

// off[0 .. n] = exclusive scan of len[0 .. n) -- len has n + 1 entries, the sentinel len[n] is zeroed here -- and, where
// `total` is given, the read-back of off[n] is put on the stream (the caller synchronises).
template <typename In>
int offsets_of(const char* scan_ws, In* len, int64_t* off, long long n, int64_t* total, hipStream_t s) {
    SL_HIP(hipMemsetAsync(len + n, 0, sizeof(In), s));
    SL_TRY(exclusive_scan(scan_ws, len, off, static_cast<size_t>(n) + 1, s));
    if (total) SL_HIP(hipMemcpyAsync(total, off + n, sizeof *total, hipMemcpyDeviceToHost, s));
    return 0;
}

// The slot through which a fields / size kernel reports its lowest bad record: atomicMin on (index << shift | code).
struct FirstBad {
    unsigned long long* d = nullptr;
    unsigned long long v = ~0ull;      // as read back; all ones: every record passed

    int arm(const char* ws, hipStream_t s) {
        SL_TRY(scratch(ws, 1, &d));
        SL_HIP(hipMemsetAsync(d, 0xff, sizeof v, s));
        return 0;
    }
    int read(hipStream_t s) {          // (the caller synchronises)
        SL_HIP(hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, s));
        return 0;
    }
    // 0 when nothing was reported, else the failure msg[code - 1] of record / line `first` + index
    template <size_t N>
    int error(int shift, long long first, const char* const (&msg)[N]) const {
        if (v == ~0ull) return 0;
        const size_t code = std::min<size_t>(std::max<size_t>(v & ((1u << shift) - 1), 1), N);
        return fail(msg[code - 1], first + static_cast<long long>(v >> shift));
    }
};

const char* const FQ_MESSAGES[] = {
    "FASTQ record %lld does not start with '@'",                    // FQ_BAD_HEADER
    "FASTQ record %lld has no '+' line",                            // FQ_BAD_PLUS
    "FASTQ record %lld: sequence and quality lengths differ",       // FQ_BAD_LENGTH
};
const char* const SAM_MESSAGES[] = {
    "SAM line %lld: fewer than 6 tab-separated fields",             // SAM_FIELDS
    "SAM line %lld: FLAG is not a 32-bit integer",                  // SAM_FLAG
    "SAM line %lld: MAPQ is not a 32-bit integer",                  // SAM_MAPQ
    "SAM line %lld: POS is not a 32-bit integer",                   // SAM_POS
    "SAM line %lld: RNAME is neither an @SQ name nor '*'",          // SAM_RNAME
    "SAM line %lld: CIGAR '*' on a kept record",                    // SAM_CIGAR_STAR
    "SAM line %lld: CIGAR does not match ([0-9]+[MIDNSHP=X])+",     // SAM_CIGAR_SYNTAX
    "SAM line %lld: CIGAR length above 2^31 - 1",                   // SAM_CIGAR_RANGE
    "SAM line %lld: CIGAR has only H and S operations",             // SAM_CIGAR_CLIPS
    "SAM line %lld: alignment end outside the 32-bit integer range",   // SAM_END
};
const char* const BAM_MESSAGES[] = {
    "BAM record %lld: record fields do not fit its block size",     // BAM_LAYOUT
    "BAM record %lld: POS is not a 32-bit integer",                 // BAM_POS
    "BAM record %lld: reference ID outside the header's reference list",   // BAM_RNAME
    "BAM record %lld: no CIGAR on a kept record",                   // BAM_CIGAR_STAR
    "BAM record %lld: CIGAR operation code above 8",                // BAM_CIGAR_OP
    "BAM record %lld: malformed tags or CG tag behind a long-CIGAR stand-in",   // BAM_TAGS
    "BAM record %lld: CIGAR length above 2^31 - 1",                 // BAM_CIGAR_RANGE
    "BAM record %lld: CIGAR has only H and S operations",           // BAM_CIGAR_CLIPS
    "BAM record %lld: alignment end outside the 32-bit integer range",     // BAM_END
};
const char* const BAMR_MESSAGES[] = {
    "BAM record %lld: record fields do not fit its block size",     // BAMR_LAYOUT
    "BAM record %lld: SEQ holds '='",                               // BAMR_SEQ
    "BAM record %lld: quality value above 93",                      // BAMR_QUAL
};
static_assert(sizeof FQ_MESSAGES / sizeof *FQ_MESSAGES == FQ_BAD_LENGTH && sizeof SAM_MESSAGES / sizeof *SAM_MESSAGES == SAM_END &&
              sizeof BAM_MESSAGES / sizeof *BAM_MESSAGES == BAM_END && sizeof BAMR_MESSAGES / sizeof *BAMR_MESSAGES == BAMR_QUAL,
              "one message per code of readers.hpp");

// Whether a device array an index took from workspace `ws` is still that workspace (null: the index holds none).
bool held(const char* ws, const void* p) { return !p || ctx().holds(ws, p); }

// ---- the line index of nbytes > 0 of text ------------------------------------------------------------------------------------

struct LineTiles {
    long long ntiles = 0;
    long long* base = nullptr;     // ntiles + 1: newlines in front of each tile, then their total
};

// tile counts, their scan, and the number of newlines of the text (synchronises, with whatever read-backs the caller
// put on the stream before)
int line_counts(const uint8_t* d_text, long long nbytes, LineTiles* T, long long* newlines, hipStream_t s) {
    T->ntiles = (nbytes + FQ_TILE - 1) / FQ_TILE;
    long long* d_count;
    SL_TRY(scratch("fq.count", static_cast<size_t>(T->ntiles) + 1, &d_count));
    SL_TRY(scratch("fq.base", static_cast<size_t>(T->ntiles) + 1, &T->base));
    SL_TRY(lines_count(d_text, nbytes, T->ntiles, d_count, s));
    int64_t total = 0;
    SL_TRY(offsets_of("fq.scan", d_count, reinterpret_cast<int64_t*>(T->base), T->ntiles, &total, s));
    SL_HIP(hipStreamSynchronize(s));
    *newlines = total;
    return 0;
}

// workspace `ws` = the starts of the newlines + 1 lines, then `nends` (1 or 2) end sentinels nbytes + 1, nbytes + 2: a
// line ends one byte in front of the next start, so the last line ends at nbytes and the ones behind it are empty
int line_starts(const char* ws, const uint8_t* d_text, long long nbytes, const LineTiles& T, long long newlines, int nends,
                long long** d_lines, hipStream_t s) {
    const long long nlines = newlines + 1;
    SL_TRY(scratch(ws, static_cast<size_t>(nlines + nends), d_lines));
    static thread_local long long h[3];    // outlives the copies: every caller synchronises before it indexes again
    h[0] = 0; h[1] = nbytes + 1; h[2] = nbytes + 2;
    SL_HIP(hipMemcpyAsync(*d_lines, h, sizeof(long long), hipMemcpyHostToDevice, s));
    SL_HIP(hipMemcpyAsync(*d_lines + nlines, h + 1, static_cast<size_t>(nends) * sizeof(long long), hipMemcpyHostToDevice, s));
    return lines_write(d_text, nbytes, T.ntiles, T.base, *d_lines, s);
}

// ---- index states ---------------------------------------------------------------------------------------------------------

// of the last sarlacc_dev_fastq_index call on this thread
struct FastqIndex {
    const uint8_t* text = nullptr;
    int64_t nbytes = 0, nrec = 0, total_bases = 0, total_name = 0;
    FqRec* rec = nullptr;          // "fq.rec"
    int64_t* off = nullptr;        // "fq.off", "fq.noff": nrec + 1 each
    int64_t* noff = nullptr;
    bool live() const { return held("fq.rec", rec) && held("fq.off", off) && held("fq.noff", noff); }
};
thread_local FastqIndex g_fq;

// of the last sarlacc_dev_sam_index / sarlacc_dev_bam_index call on this thread
struct RangesIndex {
    const uint8_t* text = nullptr;     // the SAM body or the inflated BAM
    int64_t nlines = 0, nkept = 0, name_bytes = 0;
    SamRec* rec = nullptr;         // "sam.rec"
    int* keep = nullptr;           // "sam.keep", "sam.koff", "sam.noff": nlines + 1 each
    int64_t* koff = nullptr;
    int64_t* noff = nullptr;
    bool live() const { return held("sam.rec", rec) && held("sam.keep", keep) && held("sam.koff", koff) && held("sam.noff", noff); }
};
thread_local RangesIndex g_sam;

thread_local unsigned long long g_bam_generation = 0;      // locator runs of this thread: "bam.off" belongs to the last one

// of the last sarlacc_dev_bam_reads_index call on this thread
struct BamReadsIndex {
    bool valid = false;
    const uint8_t* bam = nullptr;
    unsigned long long generation = 0;     // of the locator run whose record offsets this state points to
    long long nrec = 0, nreads = 0, used = 0;
    long long* rec_off = nullptr;          // "bam.off", nrec + 1: the last entry is `used`
    int64_t* base_off = nullptr;           // "bamr.boff", "bamr.noff", nrec + 1 each: exclusive scans over the records
    int64_t* name_off = nullptr;
    long long* read_rec = nullptr;         // "bamr.rrec", nreads + 1: record of a read, nrec behind the last
    int* keep = nullptr;                   // "bamr.keep", nrec + 1
    int64_t* aux_off = nullptr;            // "bamr.aoff", nrec + 1, a scan as base_off is; null until tags are asked for
    bool live() const {
        return valid && generation == g_bam_generation && held("bam.off", rec_off) && held("bamr.boff", base_off) &&
               held("bamr.noff", name_off) && held("bamr.rrec", read_rec) && held("bamr.keep", keep) && held("bamr.aoff", aux_off);
    }
    BamrArrays arrays() const { return BamrArrays{bam, rec_off, base_off, name_off, read_rec, aux_off}; }
};
thread_local BamReadsIndex g_bamr;

// ---- the ranges back end of SAM and BAM ---------------------------------------------------------------------------------------

// The n > 0 lines / records of a buffer -> X: fields(rec, keep, name_len, first_bad) enqueues the format's fields kernel,
// the scans give every kept record its place and its name's, and the counts and `bad` are back when it returns.
template <typename Fields>
int ranges_index(long long n, Fields&& fields, FirstBad* bad, RangesIndex* X, hipStream_t s) {
    long long* d_nlen;
    SL_TRY(scratch("sam.rec", static_cast<size_t>(n), &X->rec));
    SL_TRY(scratch("sam.keep", static_cast<size_t>(n) + 1, &X->keep));
    SL_TRY(scratch("sam.nlen", static_cast<size_t>(n) + 1, &d_nlen));
    SL_TRY(scratch("sam.koff", static_cast<size_t>(n) + 1, &X->koff));
    SL_TRY(scratch("sam.noff", static_cast<size_t>(n) + 1, &X->noff));
    SL_TRY(bad->arm("sam.bad", s));
    SL_TRY(fields(X->rec, X->keep, d_nlen, bad->d));
    SL_TRY(offsets_of("sam.scan", X->keep, X->koff, n, &X->nkept, s));
    SL_TRY(offsets_of("sam.scan", d_nlen, X->noff, n, &X->name_bytes, s));
    SL_TRY(bad->read(s));
    SL_HIP(hipStreamSynchronize(s));
    X->nlines = n;
    return 0;
}

// the name table of a SAM header: seqinfo names (code = index), then the `restricted` names not among them (code -1)
int sam_name_table(const char* ref_names, const int64_t* ref_off, int64_t n_ref, const uint8_t* restricted_mask,
                   const char* extra_names, const int64_t* extra_off, int64_t n_extra, std::vector<SamName>* table,
                   std::vector<uint8_t>* bytes) {
    const int64_t nent = n_ref + n_extra;
    uint64_t tsize = 16;
    while (tsize < 2 * static_cast<uint64_t>(nent) + 2) tsize <<= 1;
    table->assign(tsize, SamName{0, 0, -1, 0, 0, 0});
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
        for (; (*table)[slot].len >= 0; slot = (slot + 1) & tmask) {
            const SamName& E = (*table)[slot];
            if (E.hash == h && E.len == len && std::equal(src, src + len, bytes->data() + E.off)) { dup = true; break; }
        }
        if (dup) {
            if (is_ref) return fail("duplicate @SQ name '%.*s'", static_cast<int>(std::min<int64_t>(len, 200)), src);
            continue;   // a restricted name listed twice, or one that is also a seqinfo name
        }
        (*table)[slot] = SamName{h, static_cast<long long>(bytes->size()), static_cast<int>(len), is_ref ? static_cast<int>(i) : -1,
                                 is_ref ? (restricted_mask ? restricted_mask[i] != 0 : 0) : 1, 0};
        bytes->insert(bytes->end(), src, src + len);
    }
    return 0;
}

// ---- the BAM locator ----------------------------------------------------------------------------------------------------------

// What the locator found in a buffer: the offsets of the nrec records that lie wholly in it (d_off, nrec + 1 entries of
// the workspace "bam.off", the last one unset), the offset of the first record that does not (nbytes when none is cut)
// and how the chain ends there.
struct BamLocated {
    long long nrec = 0, end = 0;
    int how = BAM_CHAIN_CLEAN;
    long long* d_off = nullptr;
};

// k_bam_hops / k_bam_chain / k_bam_starts over nbytes > 0 of inflated BAM whose byte 0 starts a record, under the stage
// timers bam_hops, bam_chain and bam_starts.  The counts are back on the host when it returns; the launch that writes
// d_off is still on the stream.
int bam_locate(const uint8_t* d_bam, long long nbytes, hipStream_t s, BamLocated* out) {
    Context& c = ctx();
    for (const char* name : {"bam_hops", "bam_chain", "bam_starts"}) c.stage_reset(name);
    ++g_bam_generation;
    const long long ntiles = (nbytes + BAM_TILE - 1) / BAM_TILE;
    if (ntiles > INT_MAX) return fail("sarlacc_amd: BAM buffer too large");
    unsigned* d_table; long long* d_entry; long long* d_count; long long* d_base; long long* d_term;
    SL_TRY(scratch("bam.hops", static_cast<size_t>(nbytes), &d_table));
    SL_TRY(scratch("bam.entry", static_cast<size_t>(ntiles), &d_entry));
    SL_TRY(scratch("bam.count", static_cast<size_t>(ntiles) + 1, &d_count));
    SL_TRY(scratch("bam.base", static_cast<size_t>(ntiles) + 1, &d_base));
    SL_TRY(scratch("bam.term", 2, &d_term));
    SL_HIP(hipMemsetAsync(d_entry, 0xff, static_cast<size_t>(ntiles) * sizeof(long long), s));
    SL_HIP(hipMemsetAsync(d_term, 0xff, 2 * sizeof(long long), s));
    SL_TRY(c.stage_begin("bam_hops", s));
    SL_TRY(bam_hops(d_bam, nbytes, ntiles, d_table, s));
    SL_TRY(c.stage_end("bam_hops", s));
    SL_TRY(c.stage_begin("bam_chain", s));
    SL_TRY(bam_chain(d_table, nbytes, ntiles, d_entry, s));
    SL_TRY(c.stage_end("bam_chain", s));
    SL_TRY(c.stage_begin("bam_starts", s));
    SL_TRY(bam_starts_count(d_bam, nbytes, ntiles, d_entry, d_count, d_term, s));
    int64_t nrec = 0;
    long long term[2] = {-1, -1};
    SL_TRY(offsets_of("bam.scan", d_count, reinterpret_cast<int64_t*>(d_base), ntiles, &nrec, s));
    SL_HIP(hipMemcpyAsync(term, d_term, sizeof term, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (term[0] < 0 || term[0] > nbytes || nrec < 0) return fail("sarlacc_amd: the BAM record chain did not end (internal error)");
    SL_TRY(scratch("bam.off", static_cast<size_t>(nrec) + 1, &out->d_off));
    if (nrec > 0) SL_TRY(bam_starts_write(d_bam, nbytes, ntiles, d_entry, d_base, out->d_off, s));
    SL_TRY(c.stage_end("bam_starts", s));
    out->nrec = nrec;
    out->end = term[0];
    out->how = static_cast<int>(term[1]);
    return 0;
}

// The locator's two refusals, for a caller that found no bad record in front of the chain's end (0: none applies).
int bam_chain_end_error(const BamLocated& L, long long first_record, int at_eof) {
    if (L.how == BAM_CHAIN_SIZE) return fail("BAM record %lld: block size below 32", first_record + L.nrec);
    if (L.how == BAM_CHAIN_INCOMPLETE && at_eof) return fail("BAM record %lld: file ends inside the record", first_record + L.nrec);
    return 0;
}

// ---- BAM reads: ranges of the indexed buffer ------------------------------------------------------------------------------------

// the records a .. e that hold the reads first .. first + count of the live index, what they need (R), and where the
// next record starts
int bamr_span(long long first, long long count, BamrRange* R, int64_t* next_byte) {
    const BamReadsIndex& X = g_bamr;
    *R = BamrRange{first, count, 0, 0, 0, 0};
    if (!X.live()) return fail("sarlacc_amd: no BAM reads index on this thread (sarlacc_dev_bam_reads_index comes first)");
    if (first < 0 || count < 0 || first > X.nreads || count > X.nreads - first) return fail("sarlacc_amd: BAM read range outside the indexed buffer");
    if (X.nrec == 0) {
        *next_byte = X.used;
        return 0;
    }
    // the record after the last read of the range; everything behind the last read of the buffer goes with it
    long long e = 0;
    if (first + count == X.nreads) e = X.nrec;
    else if (first + count > 0) {
        SL_HIP(hipMemcpy(&e, X.read_rec + first + count - 1, sizeof e, hipMemcpyDeviceToHost));
        ++e;
    }
    long long a = e;
    if (count > 0) SL_HIP(hipMemcpy(&a, X.read_rec + first, sizeof a, hipMemcpyDeviceToHost));
    if (a < 0 || a > e || e > X.nrec) return fail("sarlacc_amd: BAM reads index is damaged (internal error)");
    int64_t b[2], n[2];
    long long next = 0;
    SL_HIP(hipMemcpy(&b[0], X.base_off + a, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&b[1], X.base_off + e, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&n[0], X.name_off + a, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&n[1], X.name_off + e, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&next, X.rec_off + e, sizeof next, hipMemcpyDeviceToHost));
    R->a = a; R->e = e;
    R->bases = b[1] - b[0]; R->name_bytes = n[1] - n[0];
    *next_byte = next;
    return 0;
}

// the aux offsets of the indexed buffer's records, made on the first request
int bamr_aux_index(hipStream_t s) {
    BamReadsIndex& X = g_bamr;
    if (X.aux_off || X.nrec == 0) return 0;
    long long* d_alen; int64_t* d_aoff;
    SL_TRY(scratch("bamr.alen", static_cast<size_t>(X.nrec) + 1, &d_alen));
    SL_TRY(scratch("bamr.aoff", static_cast<size_t>(X.nrec) + 1, &d_aoff));
    SL_TRY(bamr_aux_len(X.bam, X.rec_off, X.keep, X.nrec, d_alen, s));    // (it writes its own sentinel)
    SL_TRY(exclusive_scan("bamr.scan", d_alen, d_aoff, static_cast<size_t>(X.nrec) + 1, s));
    X.aux_off = d_aoff;
    return 0;
}

}  // namespace
}  // namespace sarlacc

using namespace sarlacc;

extern "C" {

// ---- FASTQ ----------------------------------------------------------------------------------------------------------------

int sarlacc_dev_fastq_index(const uint8_t* d_text, int64_t nbytes, int64_t* n_records, int64_t* total_bases,
                            int64_t* total_name_bytes, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0) return fail("sarlacc_amd: negative FASTQ size");
    hipStream_t s = static_cast<hipStream_t>(stream);
    g_fq = FastqIndex{};
    *n_records = 0; *total_bases = 0; *total_name_bytes = 0;
    // trailing blank lines do not start a record: drop them from the text (host look at the tail)
    while (nbytes > 0) {
        const int64_t k = std::min<int64_t>(nbytes, 4096);
        std::vector<uint8_t> tail(static_cast<size_t>(k));
        SL_HIP(hipMemcpyAsync(tail.data(), d_text + nbytes - k, static_cast<size_t>(k), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        int64_t cut = k;
        while (cut > 0 && (tail[cut - 1] == '\n' || tail[cut - 1] == '\r')) --cut;
        nbytes -= k - cut;
        if (cut > 0) break;
    }
    if (nbytes == 0) {
        g_fq.text = d_text;  // an empty batch is a valid result
        return 0;
    }

    LineTiles T;
    long long newlines = 0;
    SL_TRY(line_counts(d_text, nbytes, &T, &newlines, s));
    // the text no longer ends in a newline, so there is one more line than newlines.  A last
    // record whose quality line is empty lost that line with the trailing newlines: it is put
    // back as an empty virtual line (the record check still compares the two lengths).
    const long long nlines = newlines + 1;
    if (nlines % 4 != 0 && nlines % 4 != 3) return fail("FASTQ text ends inside a record (%lld lines)", nlines);
    const long long nrec = (nlines + 1) / 4;
    long long* d_lines;
    SL_TRY(line_starts("fq.lines", d_text, nbytes, T, newlines, 2, &d_lines, s));

    FastqIndex X;
    long long* d_slen; long long* d_nlen;
    FirstBad bad;
    SL_TRY(scratch("fq.rec", static_cast<size_t>(nrec), &X.rec));
    SL_TRY(scratch("fq.slen", static_cast<size_t>(nrec) + 1, &d_slen));
    SL_TRY(scratch("fq.nlen", static_cast<size_t>(nrec) + 1, &d_nlen));
    SL_TRY(scratch("fq.off", static_cast<size_t>(nrec) + 1, &X.off));
    SL_TRY(scratch("fq.noff", static_cast<size_t>(nrec) + 1, &X.noff));
    SL_TRY(bad.arm("fq.bad", s));
    SL_TRY(fq_records(d_text, d_lines, nrec, X.rec, d_slen, d_nlen, bad.d, s));
    SL_TRY(offsets_of("fq.scan", d_slen, X.off, nrec, &X.total_bases, s));
    SL_TRY(offsets_of("fq.scan", d_nlen, X.noff, nrec, &X.total_name, s));
    SL_TRY(bad.read(s));
    SL_HIP(hipStreamSynchronize(s));
    SL_TRY(bad.error(FQ_BAD_SHIFT, 1, FQ_MESSAGES));
    X.text = d_text; X.nbytes = nbytes; X.nrec = nrec;
    g_fq = X;
    *n_records = nrec; *total_bases = X.total_bases; *total_name_bytes = X.total_name;
    return 0;
}

int sarlacc_dev_fastq_split(const uint8_t* d_text, int64_t nbytes, int64_t max_records, int64_t* n_records,
                            int64_t* consumed_bytes, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0 || max_records < 0) return fail("sarlacc_amd: negative FASTQ size");
    hipStream_t s = static_cast<hipStream_t>(stream);
    *n_records = 0; *consumed_bytes = 0;
    if (nbytes == 0 || max_records == 0) return 0;
    long long* d_pos;
    SL_TRY(scratch("fq.nth", 1, &d_pos));
    LineTiles T;
    long long newlines = 0;
    SL_TRY(line_counts(d_text, nbytes, &T, &newlines, s));
    const long long k = std::min<long long>(newlines / 4, max_records);   // records whose four lines all end in a newline
    if (k == 0) return 0;
    long long pos = -1;
    SL_HIP(hipMemsetAsync(d_pos, 0xff, sizeof(long long), s));
    SL_TRY(lines_nth_newline(d_text, nbytes, T.ntiles, T.base, 4 * k, d_pos, s));
    SL_HIP(hipMemcpyAsync(&pos, d_pos, sizeof pos, hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    if (pos <= 0 || pos > nbytes) return fail("sarlacc_amd: internal error locating the end of FASTQ record %lld", k);
    *n_records = k; *consumed_bytes = pos;
    return 0;
}

int sarlacc_dev_fastq_extract(const uint8_t* d_text, uint8_t* d_seq, uint8_t* d_qual, int64_t* d_off, uint8_t* d_names,
                              int64_t* d_name_off, void* stream) {
    SL_TRY(ensure_device());
    const FastqIndex& X = g_fq;
    if (d_text != X.text || !X.live()) return fail("sarlacc_amd: sarlacc_dev_fastq_extract without a matching sarlacc_dev_fastq_index");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t noffsets = static_cast<size_t>(X.nrec) + 1;
    if (X.nrec == 0) {
        const int64_t zero = 0;
        SL_HIP(hipMemcpyAsync(d_off, &zero, sizeof zero, hipMemcpyHostToDevice, s));
        if (d_name_off) SL_HIP(hipMemcpyAsync(d_name_off, &zero, sizeof zero, hipMemcpyHostToDevice, s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    SL_HIP(hipMemcpyAsync(d_off, X.off, sizeof(int64_t) * noffsets, hipMemcpyDeviceToDevice, s));
    if (d_name_off) SL_HIP(hipMemcpyAsync(d_name_off, X.noff, sizeof(int64_t) * noffsets, hipMemcpyDeviceToDevice, s));
    Context& c = ctx();
    SL_HIP(hipEventRecord(c.ev_start, s));
    SL_TRY(fq_copy(d_text, X.rec, X.off, X.noff, X.nrec, d_seq, d_qual, d_names, s));
    SL_HIP(hipEventRecord(c.ev_stop, s));
    c.timed = true;
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- SAM and BAM -> ranges ----------------------------------------------------------------------------------------------------

int sarlacc_dev_sam_index(const uint8_t* d_text, int64_t nbytes, int64_t first_line, const char* ref_names,
                          const int64_t* ref_off, int64_t n_ref, const uint8_t* restricted_mask, const char* extra_names,
                          const int64_t* extra_off, int64_t n_extra, int use_minq, int64_t minq, int64_t* n_lines,
                          int64_t* n_kept, int64_t* kept_name_bytes, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0 || n_ref < 0 || n_extra < 0) return fail("sarlacc_amd: negative SAM size");
    if (n_ref >= INT_MAX) return fail("sarlacc_amd: too many reference names");
    hipStream_t s = static_cast<hipStream_t>(stream);
    g_sam = RangesIndex{};
    *n_lines = 0; *n_kept = 0; *kept_name_bytes = 0;
    std::vector<SamName> table;
    std::vector<uint8_t> bytes;
    SL_TRY(sam_name_table(ref_names, ref_off, n_ref, restricted_mask, extra_names, extra_off, n_extra, &table, &bytes));
    if (nbytes == 0) {
        g_sam.text = d_text;   // no lines: an empty result
        return 0;
    }

    LineTiles T;
    long long newlines = 0;
    uint8_t last = 0;
    SL_HIP(hipMemcpyAsync(&last, d_text + nbytes - 1, 1, hipMemcpyDeviceToHost, s));
    SL_TRY(line_counts(d_text, nbytes, &T, &newlines, s));
    // one more line than newlines; after a final newline that line is empty, i.e. blank
    const long long nlines = newlines + 1;
    long long* d_lines; SamName* d_table; uint8_t* d_names;
    SL_TRY(line_starts("sam.lines", d_text, nbytes, T, newlines, 1, &d_lines, s));
    SL_TRY(upload("sam.table", table.data(), table.size(), &d_table, s));
    SL_TRY(upload("sam.names", bytes.data(), bytes.size(), &d_names, s));

    RangesIndex X;
    FirstBad bad;
    SL_TRY(ranges_index(nlines, [&](SamRec* rec, int* keep, long long* name_len, unsigned long long* first_bad) {
        return sam_fields(d_text, d_lines, nlines, d_table, table.size() - 1, d_names, restricted_mask ? 1 : 0, use_minq ? 1 : 0,
                          minq, rec, keep, name_len, first_bad, s);
    }, &bad, &X, s));
    SL_TRY(bad.error(REC_BAD_SHIFT, first_line, SAM_MESSAGES));
    X.text = d_text;
    g_sam = X;
    *n_lines = newlines + (last != '\n' ? 1 : 0);
    *n_kept = X.nkept; *kept_name_bytes = X.name_bytes;
    return 0;
}

int sarlacc_dev_sam_extract(const uint8_t* d_text, int32_t* d_ref, int32_t* d_start, int32_t* d_width, uint8_t* d_strand,
                            int32_t* d_lclip, int32_t* d_rclip, uint8_t* d_names, int64_t* d_name_off, void* stream) {
    SL_TRY(ensure_device());
    const RangesIndex& X = g_sam;
    if (!d_text || d_text != X.text || !X.live()) return fail("sarlacc_amd: sarlacc_dev_sam_extract without a matching sarlacc_dev_sam_index");
    hipStream_t s = static_cast<hipStream_t>(stream);
    SL_HIP(hipMemcpyAsync(d_name_off + X.nkept, &X.name_bytes, sizeof X.name_bytes, hipMemcpyHostToDevice, s));
    if (X.nkept > 0) {
        Context& c = ctx();
        c.stage_reset("sam_scatter");
        SL_TRY(c.stage_begin("sam_scatter", s));
        SL_TRY(sam_scatter(d_text, X.rec, X.keep, X.koff, X.noff, X.nlines, d_ref, d_start, d_width, d_strand, d_lclip, d_rclip,
                           d_names, d_name_off, s));
        SL_TRY(c.stage_end("sam_scatter", s));
    }
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

int sarlacc_bam_tile_bytes(void) { return BAM_TILE; }

int sarlacc_dev_bam_index(const uint8_t* d_bam, int64_t nbytes, int64_t first_record, int at_eof, int64_t n_ref,
                          const uint8_t* restricted_mask, int use_minq, int64_t minq, int64_t* n_records, int64_t* used_bytes,
                          int64_t* n_kept, int64_t* kept_name_bytes, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0 || n_ref < 0) return fail("sarlacc_amd: negative BAM size");
    if (n_ref >= INT_MAX) return fail("sarlacc_amd: too many reference names");
    hipStream_t s = static_cast<hipStream_t>(stream);
    g_sam = RangesIndex{};
    *n_records = 0; *used_bytes = 0; *n_kept = 0; *kept_name_bytes = 0;
    if (nbytes == 0) {
        g_sam.text = d_bam;    // no records: an empty result
        return 0;
    }
    Context& c = ctx();
    c.stage_reset("bam_fields");
    BamLocated L;
    SL_TRY(bam_locate(d_bam, nbytes, s, &L));

    RangesIndex X;
    FirstBad bad;
    if (L.nrec > 0) {
        uint8_t* d_mask = nullptr;
        if (restricted_mask) SL_TRY(upload("bam.mask", restricted_mask, static_cast<size_t>(n_ref) + 1, &d_mask, s));
        SL_TRY(ranges_index(L.nrec, [&](SamRec* rec, int* keep, long long* name_len, unsigned long long* first_bad) {
            SL_TRY(c.stage_begin("bam_fields", s));
            SL_TRY(bam_fields(d_bam, L.d_off, L.nrec, n_ref, d_mask, use_minq ? 1 : 0, minq, rec, keep, name_len, first_bad, s));
            return c.stage_end("bam_fields", s);
        }, &bad, &X, s));
    }
    SL_TRY(bad.error(REC_BAD_SHIFT, first_record, BAM_MESSAGES));   // a record before the one the chain ends at: the lowest record wins
    SL_TRY(bam_chain_end_error(L, first_record, at_eof));
    X.text = d_bam;
    g_sam = X;
    *n_records = L.nrec; *used_bytes = L.end;
    *n_kept = X.nkept; *kept_name_bytes = X.name_bytes;
    return 0;
}

int sarlacc_dev_bam_extract(const uint8_t* d_bam, int32_t* d_ref, int32_t* d_start, int32_t* d_width, uint8_t* d_strand,
                            int32_t* d_lclip, int32_t* d_rclip, uint8_t* d_names, int64_t* d_name_off, void* stream) {
    // the state, the scans and the scatter are the SAM pair's
    return sarlacc_dev_sam_extract(d_bam, d_ref, d_start, d_width, d_strand, d_lclip, d_rclip, d_names, d_name_off, stream);
}

// ---- BAM -> reads -----------------------------------------------------------------------------------------------------------

int sarlacc_dev_bam_reads_index(const uint8_t* d_bam, int64_t nbytes, int64_t first_record, int at_eof, int exclude_flags,
                                int64_t* n_records, int64_t* used_bytes, int64_t* n_reads, void* stream) {
    SL_TRY(ensure_device());
    if (nbytes < 0) return fail("sarlacc_amd: negative BAM size");
    if (exclude_flags < 0 || exclude_flags > 0xffff) return fail("'exclude_flags' must lie in 0..65535");
    hipStream_t s = static_cast<hipStream_t>(stream);
    g_bamr = BamReadsIndex{};
    *n_records = 0; *used_bytes = 0; *n_reads = 0;
    if (nbytes == 0) {      // no records: an empty batch
        g_bamr.valid = true; g_bamr.bam = d_bam; g_bamr.generation = g_bam_generation;
        return 0;
    }
    Context& c = ctx();
    c.stage_reset("bam_reads_size");
    BamLocated L;
    SL_TRY(bam_locate(d_bam, nbytes, s, &L));
    const long long nrec = L.nrec;

    BamReadsIndex X;
    FirstBad bad;
    int64_t nreads = 0;
    long long* d_bases; long long* d_nlen; int64_t* d_roff;
    SL_TRY(scratch("bamr.keep", static_cast<size_t>(nrec) + 1, &X.keep));
    SL_TRY(scratch("bamr.bases", static_cast<size_t>(nrec) + 1, &d_bases));
    SL_TRY(scratch("bamr.nlen", static_cast<size_t>(nrec) + 1, &d_nlen));
    SL_TRY(scratch("bamr.roff", static_cast<size_t>(nrec) + 1, &d_roff));
    SL_TRY(scratch("bamr.boff", static_cast<size_t>(nrec) + 1, &X.base_off));
    SL_TRY(scratch("bamr.noff", static_cast<size_t>(nrec) + 1, &X.name_off));
    SL_TRY(scratch("bamr.rrec", static_cast<size_t>(nrec) + 1, &X.read_rec));
    if (nrec > 0) {
        SL_TRY(bad.arm("bamr.bad", s));
        SL_HIP(hipMemcpyAsync(L.d_off + nrec, &L.end, sizeof(long long), hipMemcpyHostToDevice, s));
        SL_TRY(c.stage_begin("bam_reads_size", s));
        SL_TRY(bamr_size(d_bam, L.d_off, nrec, static_cast<unsigned>(exclude_flags), X.keep, d_bases, d_nlen, bad.d, s));
        SL_TRY(offsets_of("bamr.scan", X.keep, d_roff, nrec, &nreads, s));
        SL_TRY(offsets_of("bamr.scan", d_bases, X.base_off, nrec, static_cast<int64_t*>(nullptr), s));
        SL_TRY(offsets_of("bamr.scan", d_nlen, X.name_off, nrec, static_cast<int64_t*>(nullptr), s));
        SL_TRY(bamr_reads(X.keep, d_roff, nrec, X.read_rec, s));
        SL_TRY(c.stage_end("bam_reads_size", s));
        SL_TRY(bad.read(s));
        SL_HIP(hipStreamSynchronize(s));
    }
    SL_TRY(bad.error(REC_BAD_SHIFT, first_record, BAMR_MESSAGES));   // a record before the one the chain ends at: the lowest record wins
    SL_TRY(bam_chain_end_error(L, first_record, at_eof));
    X.valid = true; X.bam = d_bam; X.generation = g_bam_generation;
    X.nrec = nrec; X.nreads = nreads; X.used = L.end;
    X.rec_off = L.d_off;
    g_bamr = X;
    *n_records = nrec; *used_bytes = L.end; *n_reads = nreads;
    return 0;
}

int sarlacc_dev_bam_reads_range(int64_t first, int64_t count, int64_t* total_bases, int64_t* total_name_bytes,
                                int64_t* next_byte) {
    BamrRange R;
    SL_TRY(bamr_span(first, count, &R, next_byte));
    *total_bases = R.bases; *total_name_bytes = R.name_bytes;
    return 0;
}

int sarlacc_dev_bam_reads_records(int64_t reads_taken, int64_t* n_records) {
    BamrRange R;
    int64_t next = 0;
    SL_TRY(bamr_span(0, reads_taken, &R, &next));
    *n_records = R.e;
    return 0;
}

int sarlacc_dev_bam_reads_extract(const uint8_t* d_bam, int64_t first, int64_t count, int missing_qual, uint8_t* d_seq,
                                  uint8_t* d_qual, int64_t* d_off, uint8_t* d_names, int64_t* d_name_off, void* stream) {
    if (missing_qual < 0 || missing_qual > 93) return fail("'missing_qual' must lie in 0..93");
    if ((d_names == nullptr) != (d_name_off == nullptr)) return fail("sarlacc_amd: read names and their offsets go together");
    BamrRange R;
    int64_t next = 0;
    SL_TRY(bamr_span(first, count, &R, &next));
    const BamReadsIndex& X = g_bamr;
    if (d_bam != X.bam) return fail("sarlacc_amd: not the BAM buffer indexed last on this thread");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count == 0 || X.nrec == 0) {      // offsets that start at 0, and nothing else
        SL_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), s));
        if (d_name_off) SL_HIP(hipMemsetAsync(d_name_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    Context& c = ctx();
    c.stage_reset("bam_reads_unpack");
    SL_TRY(c.stage_begin("bam_reads_unpack", s));
    SL_TRY(bamr_unpack(X.arrays(), R, missing_qual, d_seq, d_qual, d_off, d_names, d_name_off, s));
    SL_TRY(c.stage_end("bam_reads_unpack", s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}

int sarlacc_dev_bam_reads_aux_range(int64_t first, int64_t count, int64_t* aux_bytes) {
    BamrRange R;
    int64_t next = 0;
    SL_TRY(bamr_span(first, count, &R, &next));
    *aux_bytes = 0;
    if (count == 0 || g_bamr.nrec == 0) return 0;
    SL_TRY(bamr_aux_index(nullptr));
    int64_t b[2];
    SL_HIP(hipMemcpy(&b[0], g_bamr.aux_off + R.a, sizeof(int64_t), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(&b[1], g_bamr.aux_off + R.e, sizeof(int64_t), hipMemcpyDeviceToHost));
    *aux_bytes = b[1] - b[0];
    return 0;
}

int sarlacc_dev_bam_reads_aux_extract(const uint8_t* d_bam, int64_t first, int64_t count, uint8_t* d_aux, int64_t* d_aux_off,
                                      void* stream) {
    BamrRange R;
    int64_t next = 0;
    SL_TRY(bamr_span(first, count, &R, &next));
    const BamReadsIndex& X = g_bamr;
    if (d_bam != X.bam) return fail("sarlacc_amd: not the BAM buffer indexed last on this thread");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count == 0 || X.nrec == 0) {
        SL_HIP(hipMemsetAsync(d_aux_off, 0, sizeof(int64_t), s));
        SL_HIP(hipStreamSynchronize(s));
        return 0;
    }
    SL_TRY(bamr_aux_index(s));
    Context& c = ctx();
    c.stage_reset("bam_reads_aux");
    SL_TRY(c.stage_begin("bam_reads_aux", s));
    SL_TRY(bamr_aux(X.arrays(), R, d_aux, d_aux_off, s));
    SL_TRY(c.stage_end("bam_reads_aux", s));
    SL_HIP(hipStreamSynchronize(s));
    return 0;
}
}
