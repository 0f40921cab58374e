// align_host.hpp -- the host side of align.hip that align_panel.hip builds on: the cost table layout, the batch upload,
// run_align itself and its error order (one reference against a batch, any length).
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

int column_info(char r, uint32_t* info);
void build_tables(const double* errors, int n, std::vector<double>& tab);
void build_cost_rows(const std::vector<double>& tab, int n, const uint32_t* colinfo, int R, std::vector<double>& rows,
                     std::vector<uint32_t>& colbase);
int upload_batch(const char* seq, const int64_t* seq_off, const char* qual, const int64_t* qual_off, int64_t n, HostBatch* hb,
                 hipStream_t s, bool defer_data = false);
int run_align(const uint8_t* d_seq, const uint8_t* d_nmask, const uint8_t* d_qual, const int64_t* d_off, int64_t n,
              int32_t max_len, const double* enc_errors, const char* enc_names, int enc_n, double gapopen, double gapext,
              const char* ref, int R, bool local, int kernel_mode, const int32_t* sec_starts, const int32_t* sec_ends, int nsec,
              const AlignOut& out, hipStream_t stream, int* bad_qual_read, const ChunkOpts& co = ChunkOpts());
// The error the reference's loop over the reads would raise first (0: none), given the host offsets of the batch
// (qual_off NULL: lengths agree) and the bad-quality read run_align reported.
int first_error(int64_t n, const int64_t* seq_off, const int64_t* qual_off, const char* ref, int R, int bad_qual_read);

}  // namespace sarlacc
