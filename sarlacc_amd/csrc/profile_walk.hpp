// profile_walk.hpp -- the wave-wide walk over one gapped string that the profiling kernels share (profile.hip,
// profile_reads.hip): lane masks of a 64-character step and the runs of a string as the wave meets their ends.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sarlacc {

constexpr int PF_WAVES = 4;   // strings per workgroup

__device__ __forceinline__ int pf_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned long long pf_below(int lane) { return (1ull << lane) - 1ull; }
// highest set bit of m below `lane`, -1 if none
__device__ __forceinline__ int pf_prev(unsigned long long m, int lane) {
    const unsigned long long b = m & pf_below(lane);
    return b ? 63 - __builtin_clzll(b) : -1;
}

// The runs of one string, as the wave meets their ends.  emit(lane_is_emitting, start index, index of the next run's
// first character (or the string length), position in the ungapped string, bases in the run, base, index after the
// previous non-gap character (the run's start extended over the gaps before it), index after the run's last base):
// called once per step and once for the run that is open at the end, with every lane taking part.
template <typename Emit>
__device__ __forceinline__ void pf_runs(const uint8_t* s, long long len, Emit emit) {
    const int lane = pf_lane();
    // the open run: its base (0: none yet), first index, ungapped position, bases so far, index after the non-gap character
    // before it; plus the ungapped characters and the index after the last non-gap character seen so far
    int cbase = 0;
    long long cstart = 0, cpos = 0, clen = 0, cfar = 0, ung = 0, lastng = 0;
    for (long long x0 = 0; x0 < len; x0 += 64) {
        const long long x = x0 + lane;
        const int c = x < len ? s[x] : '-';
        const bool ng = c != '-';
        const unsigned long long m_ng = __ballot(ng);
        const int pl = pf_prev(m_ng, lane);
        const int pc_lane = __shfl(c, pl < 0 ? 0 : pl);
        const int prevc = pl < 0 ? cbase : pc_lane;
        const bool st = ng && prevc != c;
        const unsigned long long m_st = __ballot(st);
        // a start at lane t closes the run before it: the one that started at the previous start of this step, or the open one
        const int u = pf_prev(m_st, lane);
        const long long u_pos = ung + __popcll(m_ng & pf_below(u < 0 ? 0 : u));
        const long long u_len = __popcll(m_ng & pf_below(lane) & ~pf_below(u < 0 ? 0 : u));
        const int u_base = __shfl(c, u < 0 ? 0 : u);
        const int u_pl = __shfl(pl, u < 0 ? 0 : u);                      // the non-gap lane before the run's first base
        const long long u_far = u_pl < 0 ? lastng : x0 + u_pl + 1;
        const bool from_open = u < 0;
        const bool fire = st && (!from_open || cbase != 0);
        const long long e_start = from_open ? cstart : x0 + u;
        const long long e_pos = from_open ? cpos : u_pos;
        const long long e_len = from_open ? clen + __popcll(m_ng & pf_below(lane)) : u_len;
        const int e_base = from_open ? cbase : u_base;
        const long long e_far = from_open ? cfar : u_far;
        const long long e_right = pl < 0 ? lastng : x0 + pl + 1;          // index after the last base before this start
        emit(fire, e_start, x, e_pos, e_len, e_base, e_far, e_right);
        // what stays open
        if (m_st) {
            const int t = 63 - __builtin_clzll(m_st);
            const int t_pl = __shfl(pl, t);
            cbase = __shfl(c, t);
            cstart = x0 + t;
            cpos = ung + __popcll(m_ng & pf_below(t));
            clen = __popcll(m_ng & ~pf_below(t));
            cfar = t_pl < 0 ? lastng : x0 + t_pl + 1;
        } else {
            clen += __popcll(m_ng);
        }
        ung += __popcll(m_ng);
        if (m_ng) lastng = x0 + (63 - __builtin_clzll(m_ng)) + 1;
    }
    emit(lane == 0 && cbase != 0, cstart, len, cpos, clen, cbase, cfar, lastng);
}

}  // namespace sarlacc
