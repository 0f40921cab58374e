// sam_rec.hpp -- what the SAM text parser (sam.hip) and the BAM record parser (bam.hip) share: the per-record result
// that their field kernels fill, and the state that either index call leaves for the extract step (the keep / scan /
// scatter back end lives in sam.hip and serves both).
#pragma once

#include <cstdint>

namespace sarlacc {

// per line / record; written for kept ones only
struct SamRec {
    long long name_pos;
    int ref, start, width, lclip, rclip, strand;
};

// state of the last sarlacc_dev_sam_index / sarlacc_dev_bam_index call on this thread
struct SamIndex {
    const uint8_t* text = nullptr;
    int64_t nlines = 0, nkept = 0, name_bytes = 0;
};
extern thread_local SamIndex g_sam;

}  // namespace sarlacc
