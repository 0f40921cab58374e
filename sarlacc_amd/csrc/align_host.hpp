// align_host.hpp -- what align.hip (the kernels, their launch plan, run_align), align_host.cpp (tables, batch upload, error
// order, the C entry points) and their callers align_panel.hip / profile_reads.hip share: one reference against a batch,
// any length.
#pragma once

#include "common.hpp"

namespace sarlacc {

struct AlignOut {
    double* d_scores = nullptr;
    int32_t* d_starts = nullptr;
    int32_t* d_ends = nullptr;
    int32_t* d_sec_so = nullptr;
    int32_t* d_sec_wo = nullptr;
    // mode 2
    uint8_t* d_aln_ref = nullptr;
    uint8_t* d_aln_qry = nullptr;
    int32_t* d_aln_len = nullptr;
    int32_t* d_edits = nullptr;
};

// A host call may hand its batch over in chunks so that the upload of chunk k+1 overlaps the
// kernel of chunk k: every chunk is one run_align on a slice of the same device arrays.
struct ChunkOpts {
    int64_t sec_stride = 0;   // 0: n (stand-alone launch)
    int read_base = 0;        // index of the slice's first read in the whole batch
    bool init_bad = true;     // reset the bad-quality flag (first chunk only)
    bool finish = true;       // read the flag back and wait for the stream (last chunk only)
    const char* stage = nullptr;   // time the launch as one more segment of this stage timer instead of the call's event pair
};

struct HostBatch {
    uint8_t* d_seq = nullptr;
    uint8_t* d_qual = nullptr;
    int64_t* d_off = nullptr;
    int32_t max_len = 0;
    int64_t len_bad = -1;
};

// One run_align: a batch on the device against one reference.
struct AlignBatch {
    const uint8_t* d_seq = nullptr;     // ASCII bases, or 2-bit packed bases with d_nmask
    const uint8_t* d_qual = nullptr;
    const int64_t* d_off = nullptr;
    int64_t n = 0;
    int32_t max_len = 0;
    const uint8_t* d_nmask = nullptr;   // packed input only (sarlacc_dev_pack_reads)
};
struct AlignScoring {
    const double* enc_errors = nullptr;
    const char* enc_names = nullptr;
    int enc_n = 0;
    double gapopen = 0, gapext = 0;
};
struct AlignJob {
    AlignBatch batch;
    AlignScoring sc;
    const char* ref = nullptr;
    int R = 0;
    bool local = false;
    int kernel_mode = 0;   // 0 scores, 1 map, 2 strings
    const int32_t* sec_starts = nullptr;
    const int32_t* sec_ends = nullptr;
    int nsec = 0;
    AlignOut out;
    hipStream_t stream = nullptr;
};

int column_info(char r, uint32_t* info);
void build_tables(const double* errors, int n, std::vector<double>& tab);
void build_cost_rows(const std::vector<double>& tab, int n, const uint32_t* colinfo, int R, std::vector<double>& rows,
                     std::vector<uint32_t>& colbase);
int upload_batch(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t n, HostBatch* hb,
                 hipStream_t s, bool defer_data = false);
// Returns in *bad_qual_read the smallest index of a read with a quality character below the encoding offset (or INT_MAX).
int run_align(const AlignJob& job, int* bad_qual_read, const ChunkOpts& co = ChunkOpts());
// Workgroups of `waves` wavefronts for `nitems` wavefront-sized work items: run_align's grid policy (align.hip)
long long align_grid(long long nitems, int waves, int num_cu);
// The error the reference's loop over the reads would raise first (0: none), given the host offsets of the batch
// (qual_off NULL: lengths agree) and the bad-quality read run_align reported.
int first_error(int64_t n, const int64_t* seq_off, const int64_t* qual_off, const char* ref, int R, int bad_qual_read);

}  // namespace sarlacc
