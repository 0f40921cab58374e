// devprim.hpp -- device-wide primitives shared by the modules: rocprim sorts and scans whose temporary storage is a
// named workspace buffer (the caller names it, see Context::buffer), and launch-size helpers.
#pragma once

#include "common.hpp"

#include <rocprim/rocprim.hpp>

#include <string>

namespace sarlacc {

// blocks of `bs` threads that cover n items
inline unsigned nblk(long long n, int bs) { return static_cast<unsigned>((n + bs - 1) / bs); }

// largest r in [lo, hi) with a[r] <= g, given a[lo] <= g: the string of a flat layout that holds byte g
__device__ __forceinline__ long long last_not_above(const int64_t* a, long long lo, long long hi, long long g) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// bits a radix sort needs for keys below x (at least 1)
inline int ceil_log2(unsigned long long x) {
    int b = 1;
    while (b < 64 && (1ull << b) < x) ++b;
    return b;
}

// out[i] = in[0] + ... + in[i - 1], summed in the output's type
template <typename In, typename Out>
int exclusive_scan(const std::string& ws, const In* in, Out* out, size_t n, hipStream_t s) {
    size_t tmp = 0;
    SL_HIP(rocprim::exclusive_scan(nullptr, tmp, in, out, static_cast<Out>(0), n, rocprim::plus<Out>(), s));
    void* d_tmp;
    SL_TRY(ctx().buffer(ws.c_str(), tmp ? tmp : 16, &d_tmp));
    SL_HIP(rocprim::exclusive_scan(d_tmp, tmp, in, out, static_cast<Out>(0), n, rocprim::plus<Out>(), s));
    return 0;
}

// stable LSD radix sorts on the low `bits` bits of the keys
template <typename K>
int radix_sort_keys(const std::string& ws, K* in, K* out, size_t n, int bits, hipStream_t s) {
    size_t tmp = 0;
    SL_HIP(rocprim::radix_sort_keys(nullptr, tmp, in, out, n, 0, bits, s));
    void* d_tmp;
    SL_TRY(ctx().buffer(ws.c_str(), tmp ? tmp : 16, &d_tmp));
    SL_HIP(rocprim::radix_sort_keys(d_tmp, tmp, in, out, n, 0, bits, s));
    return 0;
}

template <typename K, typename V>
int radix_sort_pairs(const std::string& ws, K* kin, K* kout, V* vin, V* vout, size_t n, int bits, hipStream_t s) {
    size_t tmp = 0;
    SL_HIP(rocprim::radix_sort_pairs(nullptr, tmp, kin, kout, vin, vout, n, 0, bits, s));
    void* d_tmp;
    SL_TRY(ctx().buffer(ws.c_str(), tmp ? tmp : 16, &d_tmp));
    SL_HIP(rocprim::radix_sort_pairs(d_tmp, tmp, kin, kout, vin, vout, n, 0, bits, s));
    return 0;
}

}  // namespace sarlacc
