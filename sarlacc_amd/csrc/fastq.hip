// fastq.hip -- FASTQ text -> resident read batch, on gfx950.
//
// The reference streams the file through ShortRead::FastqStreamer and converts every chunk
// to a QualityScaledDNAStringSet on the host (/root/reference/R/adaptorAlign.R:26-37,
// .FASTQ2QSDS :104-110; again in R/realizeReads.R:15-26).  Here the raw text is copied to
// HBM once and parsed there; sequences, qualities, offsets and read names come out in the
// flat layout every other kernel of the library consumes, without a host-side pass over
// the bases.
//
//   (the line index: k_fq_count, scan, k_fq_lines of text_lines.hip)
//   k_fq_records  per 4-line record: checks '@' / '+' / equal lengths, strips CR, lengths;
//                 a bad record by atomicMin on (record << 3 | code)
//   (rocPRIM exclusive scans of the sequence and name lengths)
//   k_fq_copy     sequence (upper-cased), quality and name bytes -> contiguous arrays
//
// Streaming byte work, HBM-bound: ~2 reads + 1 write of the text.  The host side -- the three sarlacc_dev_fastq_*
// entry points, workspaces, scans, messages -- is in readers_host.cpp; the two functions at the end only enqueue.
#include "devprim.hpp"
#include "readers.hpp"
#include "text_lines.hpp"

#include <algorithm>

namespace sarlacc {

__global__ void k_fq_records(const uint8_t* text, const long long* line_start, long long nrec, FqRec* rec,
                             long long* seq_len, long long* name_len, unsigned long long* first_bad) {
    const long long r = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    if (r >= nrec) return;
    long long b[4], e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[k] = line_start[4 * r + k];
        e[k] = line_start[4 * r + k + 1] - 1;               // the newline (or the end of the text)
        if (e[k] > b[k] && text[e[k] - 1] == '\r') --e[k];  // CRLF files
    }
    int bad = 0;
    if (e[0] <= b[0] || text[b[0]] != '@') bad = FQ_BAD_HEADER;
    else if (e[2] <= b[2] || text[b[2]] != '+') bad = FQ_BAD_PLUS;
    else if (e[1] - b[1] != e[3] - b[3]) bad = FQ_BAD_LENGTH;
    if (bad) atomicMin(first_bad, (static_cast<unsigned long long>(r) << 3) | static_cast<unsigned>(bad));
    rec[r].seq_pos = b[1];
    rec[r].qual_pos = b[3];
    rec[r].name_pos = b[0] + 1;
    seq_len[r] = bad ? 0 : e[1] - b[1];
    name_len[r] = bad ? 0 : e[0] - b[0] - 1;
}

// a-z -> A-Z on four packed bytes
__device__ __forceinline__ uint32_t upper4(uint32_t w) {
    uint32_t out = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t c = (w >> (8 * b)) & 0xffu;
        if (c - 'a' < 26u) c -= 32u;
        out |= c << (8 * b);
    }
    return out;
}

template <bool UPPER>
__device__ __forceinline__ void copy_bytes(const uint8_t* src, uint8_t* dst, long long len, int tid, int nthreads) {
    const long long words = len >> 2;
    for (long long p = tid; p < words; p += nthreads) {
        uint32_t v = *reinterpret_cast<const u32_unaligned*>(src + 4 * p);
        if (UPPER) v = upper4(v);
        *reinterpret_cast<u32_unaligned*>(dst + 4 * p) = v;
    }
    for (long long p = 4 * words + tid; p < len; p += nthreads) {
        uint8_t c = src[p];
        if (UPPER && static_cast<unsigned>(c - 'a') < 26u) c -= 32;
        dst[p] = c;
    }
}

__global__ void __launch_bounds__(128) k_fq_copy(const uint8_t* text, const FqRec* rec, const int64_t* off,
                                                 const int64_t* name_off, long long nrec, uint8_t* seq, uint8_t* qual,
                                                 uint8_t* names) {
    for (long long r = blockIdx.x; r < nrec; r += gridDim.x) {
        const FqRec R = rec[r];
        const long long o = off[r], len = off[r + 1] - o;
        copy_bytes<true>(text + R.seq_pos, seq + o, len, threadIdx.x, blockDim.x);
        copy_bytes<false>(text + R.qual_pos, qual + o, len, threadIdx.x, blockDim.x);
        if (names) {
            const long long no = name_off[r];
            copy_bytes<false>(text + R.name_pos, names + no, name_off[r + 1] - no, threadIdx.x, blockDim.x);
        }
    }
}

int fq_records(const uint8_t* text, const long long* line_start, long long nrec, FqRec* rec, long long* seq_len,
               long long* name_len, unsigned long long* first_bad, hipStream_t s) {
    hipLaunchKernelGGL(k_fq_records, dim3(nblk(nrec, 256)), dim3(256), 0, s, text, line_start, nrec, rec, seq_len, name_len,
                       first_bad);
    SL_HIP(hipGetLastError());
    return 0;
}

int fq_copy(const uint8_t* text, const FqRec* rec, const int64_t* off, const int64_t* name_off, long long nrec, uint8_t* seq,
            uint8_t* qual, uint8_t* names, hipStream_t s) {
    // one workgroup per record (up to 1024 per CU): dynamic dispatch beats a resident grid with a stride
    const unsigned grid = static_cast<unsigned>(std::min<long long>(nrec, static_cast<long long>(ctx().num_cu) * 1024));
    hipLaunchKernelGGL(k_fq_copy, dim3(grid), dim3(128), 0, s, text, rec, off, name_off, nrec, seq, qual, names);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
