// read_groups.hip -- per-read pre-groups from alignment records (generics.readGroups), on gfx950: the records of
// sam2ranges are joined to the reads of a batch by name, one record is chosen per read, and the reads are labelled by
// reference or by overlap of their chosen ranges.  The host side (read_groups_host.cpp) runs the rocPRIM sorts and scans
// between these launches.
//
//   k_name_keys     one wavefront per read name, 64 bytes per step: the key ends in front of the first space or tab
//                   (a ballot), its 64-bit hash is the sum over its bytes of a mixed (position, byte) word, reduced
//                   across the lanes -- no serial loop over the bytes.
//   k_name_build    one wavefront per read: open addressing with linear probing over >= 2 n slots of tag << 32 | read.
//                   A free slot is claimed by compare-and-swap; a slot that holds the SAME key (tag, length and every
//                   byte equal) is lowered by atomicMin.  A key never takes two slots (every read of a key walks the same
//                   chain and slots are never freed), so each slot ends with the lowest read of its key whatever the
//                   arrival order.  Which slot a key takes does depend on the order; nothing that is returned does.
//   k_name_check    every read looks its own key up; one that finds a lower read reports read << 32 | found (atomicMin):
//                   the duplicate with the lowest index and the first read of its key.
//   k_name_probe    one wavefront per record name (whole, no cut): same hash, same chain, -1 at the first free slot.
//                   Equality is decided by the bytes; tag and length only spare a comparison.
//   k_pick_max / k_pick_decode   per record one 64-bit atomicMax on width << 32 | (0xffffffff - row) into its read's word:
//                   the widest row, the lowest among equals; a 32-bit atomicAdd counts the rows.
//   k_locus_keys / k_locus_ends / k_locus_flags / k_locus_scatter   sort key (reference, strand bit, start) per read, the
//                   ends in sorted order, the group heads from the segmented running maximum, the labels in read order.
//   k_csr_keys / k_csr_heads / k_csr_offsets   labels -> (label, 1-based index) pairs, run heads, group offsets.
//
// Memory: a name is read only inside [off[r], off[r + 1]), and only after 0 <= off[r] <= off[r + 1] <= off[n] has been
// seen for it (a name that fails is handled as the empty string and reported); every load is of one byte, so the last
// name of a buffer of exact size is read like any other.  No kernel waits on another workgroup; the probing loops end
// after nslots steps at the latest (the table is never more than half full).  A bad value is an error return
// (RgState), never a trap.
#include "read_groups.hpp"

#include "devprim.hpp"

#include <algorithm>

namespace sarlacc {
namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / 64;

__device__ __forceinline__ uint64_t mix_byte(unsigned b, long long pos) {
    uint64_t t = ((static_cast<uint64_t>(pos) << 8) | b) + 1;
    t *= 0x9E3779B97F4A7C15ull;
    t ^= t >> 32;
    t *= 0xD6E8FEB86659FD93ull;
    t ^= t >> 29;
    return t;
}

// [begin, begin + len) of name r, len = 0 and *bad set where the offsets do not ascend inside the buffer
__device__ __forceinline__ long long name_span(const NameSet& S, long long r, long long* len, bool* bad) {
    const long long a = S.off[r], b = S.off[r + 1], total = S.off[S.n];
    *bad = a < 0 || b < a || b > total || b - a > 0x7fffffffLL;
    *len = *bad ? 0 : b - a;
    return *bad ? 0 : a;
}

// key length and hash of the name s[0 .. len), the same in every lane; cut: the key ends in front of the first space or tab
__device__ __forceinline__ uint64_t wave_name_key(const uint8_t* s, long long len, bool cut, int hash_bits, int lane, long long* klen) {
    uint64_t acc = 0;
    long long kl = len;
    for (long long p0 = 0; p0 < len; p0 += 64) {
        const long long p = p0 + lane;
        const unsigned b = p < len ? s[p] : 0u;
        const unsigned long long stop = __ballot(cut && p < len && (b == ' ' || b == '\t'));
        const int first = stop ? __ffsll(static_cast<long long>(stop)) - 1 : 64;
        if (p < len && lane < first) acc += mix_byte(b, p);
        if (stop) { kl = p0 + first; break; }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) acc += __shfl_xor(acc, d);
    acc += static_cast<uint64_t>(kl) * 0xC2B2AE3D27D4EB4Full;
    acc ^= acc >> 33;
    acc *= 0xFF51AFD7ED558CCDull;
    acc ^= acc >> 33;
    if (hash_bits > 0 && hash_bits < 64) acc &= (1ull << hash_bits) - 1;
    *klen = kl;
    return acc;
}

__device__ __forceinline__ bool wave_bytes_equal(const uint8_t* a, const uint8_t* b, long long len, int lane) {
    for (long long p0 = 0; p0 < len; p0 += 64) {
        const long long p = p0 + lane;
        if (__ballot(p < len && a[p] != b[p])) return false;
    }
    return true;
}

__device__ __forceinline__ uint64_t slot_load(const uint64_t* slot) { return __atomic_load_n(slot, __ATOMIC_RELAXED); }

#define RG_WAVE_LOOP(r, n)                                                                                     \
    const int lane = threadIdx.x & 63;                                                                         \
    const long long nwaves__ = static_cast<long long>(gridDim.x) * RG_WAVES;                                   \
    for (long long r = static_cast<long long>(blockIdx.x) * RG_WAVES + (threadIdx.x >> 6); r < (n); r += nwaves__)

__global__ void __launch_bounds__(RG_THREADS) k_name_keys(NameSet R, int hash_bits, int32_t* klen, uint64_t* hash, RgState* st) {
    RG_WAVE_LOOP(i, R.n) {
        long long len, kl;
        bool bad;
        const long long a = name_span(R, i, &len, &bad);
        const uint64_t h = wave_name_key(R.chars + a, len, true, hash_bits, lane, &kl);
        if (lane == 0) {
            klen[i] = static_cast<int32_t>(kl);
            hash[i] = h;
            if (bad) atomicMin(&st->bad_read_off, static_cast<unsigned long long>(i));
        }
    }
}

__global__ void __launch_bounds__(RG_THREADS) k_name_build(NameSet R, const int32_t* klen, const uint64_t* hash, uint64_t* table,
                                                           long long nslots) {
    const uint64_t smask = static_cast<uint64_t>(nslots) - 1;
    RG_WAVE_LOOP(i, R.n) {
        const uint64_t h = hash[i], mine = (h & 0xffffffff00000000ull) | static_cast<uint64_t>(i);
        const int32_t kl = klen[i];
        const uint8_t* key = R.chars + R.off[i];      // (kl bytes: 0 where the offsets are bad, so never dereferenced then)
        uint64_t slot = h & smask;
        for (long long step = 0; step < nslots; ++step, slot = (slot + 1) & smask) {
            uint64_t cur = 0;
            if (lane == 0) {
                cur = slot_load(table + slot);
                if (cur == RG_EMPTY) {
                    cur = atomicCAS(reinterpret_cast<unsigned long long*>(table + slot), RG_EMPTY, mine);
                    if (cur == RG_EMPTY) cur = mine;      // claimed
                }
            }
            cur = __shfl(cur, 0);
            if (cur == mine) break;
            if ((cur >> 32) != (mine >> 32)) continue;
            const long long j = static_cast<long long>(cur & 0xffffffffull);
            if (j >= R.n || klen[j] != kl) continue;
            if (!wave_bytes_equal(key, R.chars + R.off[j], kl, lane)) continue;
            if (lane == 0) atomicMin(reinterpret_cast<unsigned long long*>(table + slot), mine);
            break;
        }
    }
}

__global__ void __launch_bounds__(RG_THREADS) k_name_check(NameSet R, const int32_t* klen, const uint64_t* hash,
                                                           const uint64_t* table, long long nslots, RgState* st) {
    const uint64_t smask = static_cast<uint64_t>(nslots) - 1;
    RG_WAVE_LOOP(i, R.n) {
        const uint64_t h = hash[i];
        const int32_t kl = klen[i];
        const uint8_t* key = R.chars + R.off[i];
        uint64_t slot = h & smask;
        for (long long step = 0; step < nslots; ++step, slot = (slot + 1) & smask) {
            const uint64_t cur = table[slot];
            if (cur == RG_EMPTY) break;                   // (not reached: the build put the key in front of it)
            if ((cur >> 32) != (h >> 32)) continue;
            const long long j = static_cast<long long>(cur & 0xffffffffull);
            if (j == i) break;
            if (j >= R.n || klen[j] != kl) continue;
            if (!wave_bytes_equal(key, R.chars + R.off[j], kl, lane)) continue;
            if (lane == 0) atomicMin(&st->dup, (static_cast<unsigned long long>(i) << 32) | static_cast<unsigned long long>(j));
            break;
        }
    }
}

__global__ void __launch_bounds__(RG_THREADS) k_name_probe(NameSet R, const int32_t* klen, const uint64_t* table, long long nslots,
                                                           NameSet Q, int hash_bits, int32_t* read_of_record, RgState* st) {
    const uint64_t smask = static_cast<uint64_t>(nslots) - 1;
    unsigned long long missed = 0, bad_first = ~0ull;
    RG_WAVE_LOOP(r, Q.n) {
        long long len, kl;
        bool bad;
        const long long a = name_span(Q, r, &len, &bad);
        const uint8_t* name = Q.chars + a;
        const uint64_t h = wave_name_key(name, len, false, hash_bits, lane, &kl);
        int32_t found = -1;
        uint64_t slot = h & smask;
        for (long long step = 0; !bad && R.n > 0 && step < nslots; ++step, slot = (slot + 1) & smask) {
            const uint64_t cur = table[slot];
            if (cur == RG_EMPTY) break;
            if ((cur >> 32) != (h >> 32)) continue;
            const long long j = static_cast<long long>(cur & 0xffffffffull);
            if (j >= R.n || klen[j] != kl) continue;
            if (!wave_bytes_equal(name, R.chars + R.off[j], kl, lane)) continue;
            found = static_cast<int32_t>(j);
            break;
        }
        if (lane == 0) read_of_record[r] = found;
        if (found < 0) ++missed;
        if (bad && static_cast<unsigned long long>(r) < bad_first) bad_first = static_cast<unsigned long long>(r);
    }
    // one add per workgroup
    __shared__ unsigned long long block_missed;
    if (threadIdx.x == 0) block_missed = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (missed) atomicAdd(&block_missed, missed);
        if (bad_first != ~0ull) atomicMin(&st->bad_rec_off, bad_first);
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_missed) atomicAdd(&st->unmatched, block_missed);
}

// ---- pick ----
__global__ void __launch_bounds__(256) k_pick_max(const int32_t* read_of_record, const int32_t* width, long long n_records,
                                                  long long n_reads, unsigned long long* best, int32_t* count, RgState* st) {
    const long long r = blockIdx.x * 256LL + threadIdx.x;
    if (r >= n_records) return;
    const long long i = read_of_record[r];
    if (i < 0) return;
    const int32_t w = width[r];
    if (i >= n_reads || w < 0) { atomicMin(&st->bad_value, static_cast<unsigned long long>(r)); return; }
    atomicMax(best + i, (static_cast<unsigned long long>(w) << 32) | (0xffffffffull - static_cast<unsigned long long>(r)));
    atomicAdd(count + i, 1);
}

__global__ void __launch_bounds__(256) k_pick_decode(const unsigned long long* best, long long n_reads, int32_t* record_of_read) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n_reads) return;
    const unsigned long long b = best[i];      // 0: no row (a row's low word is at least 0x80000000)
    record_of_read[i] = b ? static_cast<int32_t>(0xffffffffull - (b & 0xffffffffull)) : -1;
}

// ---- locus ----
__device__ __forceinline__ int32_t key_start(uint64_t key) { return static_cast<int32_t>(static_cast<uint32_t>(key) ^ 0x80000000u); }

__global__ void __launch_bounds__(256) k_locus_keys(LocusArgs a, uint64_t* key, int32_t* idx, RgState* st) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= a.n_reads) return;
    const long long rec = a.record_of_read[i];
    uint64_t k = RG_UNMAPPED;
    if (rec >= 0) {
        const long long ref = rec < a.n_records ? a.ref[rec] : -1;
        if (ref < 0 || ref >= RG_MAX_REF || a.width[rec] < 0) {
            atomicMin(&st->bad_value, static_cast<unsigned long long>(i));
        } else {
            const uint64_t sbit = !a.ignore_strand && a.strand[rec] == '-' ? 1 : 0;
            k = (static_cast<uint64_t>(ref) << 33) | (sbit << 32) | (static_cast<uint32_t>(a.start[rec]) ^ 0x80000000u);
        }
    }
    key[i] = k;
    idx[i] = static_cast<int32_t>(i);
}

// per sorted position: the segment (reference, strand) and the end of the range, in 64 bits
__global__ void __launch_bounds__(256) k_locus_ends(LocusArgs a, const uint64_t* skey, const int32_t* sidx, uint32_t* seg, int64_t* end) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j >= a.n_reads) return;
    const uint64_t k = skey[j];
    seg[j] = static_cast<uint32_t>(k >> 32);
    long long e = INT64_MIN;
    if (!(k & RG_UNMAPPED)) e = static_cast<long long>(key_start(k)) + a.width[a.record_of_read[sidx[j]]] - 1;   // (checked by k_locus_keys)
    end[j] = e;
}

// flag[j]: position j starts a group; flag[n] = 0 closes the scan
__global__ void __launch_bounds__(256) k_locus_flags(LocusArgs a, const uint64_t* skey, const uint32_t* seg, const int64_t* runmax,
                                                     int32_t* flag) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j > a.n_reads) return;
    int f = 0;
    if (j < a.n_reads && !(skey[j] & RG_UNMAPPED))
        f = j == 0 || seg[j] != seg[j - 1] || static_cast<long long>(key_start(skey[j])) > runmax[j - 1] + a.maxgap;
    flag[j] = f;
}

__global__ void __launch_bounds__(256) k_locus_scatter(LocusArgs a, const uint64_t* skey, const int32_t* sidx, const int32_t* flag,
                                                       const int32_t* before, int32_t* label, RgState* st) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j > a.n_reads) return;
    if (j == a.n_reads) { st->n_groups = before[j]; return; }
    label[sidx[j]] = (skey[j] & RG_UNMAPPED) ? -1 : before[j] + flag[j] - 1;
}

// ---- labels -> CSR ----
__global__ void __launch_bounds__(256) k_csr_keys(const int32_t* label, long long n, uint32_t* key, int32_t* member) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    key[i] = label[i] < 0 ? RG_NO_LABEL : static_cast<uint32_t>(label[i]);
    member[i] = static_cast<int32_t>(i + 1);
}

__global__ void __launch_bounds__(256) k_csr_heads(const uint32_t* skey, long long n, int32_t* head) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j > n) return;
    head[j] = j < n && skey[j] != RG_NO_LABEL && (j == 0 || skey[j] != skey[j - 1]);
}

__global__ void __launch_bounds__(256) k_csr_offsets(const uint32_t* skey, long long n, const int32_t* head, const int32_t* before,
                                                     int64_t* group_off, RgState* st) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j > n) return;
    if (head[j]) group_off[before[j]] = j;
    // the one position where the members end: behind the last labelled item
    if ((j == n || skey[j] == RG_NO_LABEL) && (j == 0 || skey[j - 1] != RG_NO_LABEL)) {
        group_off[before[j]] = j;
        st->n_groups = before[j];
        st->n_members = j;
    }
}

unsigned wave_grid(long long n) {
    return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(nblk(n, RG_WAVES), static_cast<long long>(ctx().num_cu) * 16)));
}

}  // namespace

int rg_state_reset(RgState* d_state, hipStream_t s) {
    SL_HIP(hipMemsetAsync(d_state, 0, sizeof(RgState), s));
    SL_HIP(hipMemsetAsync(d_state, 0xff, 4 * sizeof(unsigned long long), s));      // dup and the three bad_*
    return 0;
}

int launch_name_keys(NameSet reads, int hash_bits, int32_t* klen, uint64_t* hash, RgState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_name_keys, dim3(wave_grid(reads.n)), dim3(RG_THREADS), 0, s, reads, hash_bits, klen, hash, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_name_build(NameSet reads, const int32_t* klen, const uint64_t* hash, uint64_t* table, long long nslots, hipStream_t s) {
    hipLaunchKernelGGL(k_name_build, dim3(wave_grid(reads.n)), dim3(RG_THREADS), 0, s, reads, klen, hash, table, nslots);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_name_check(NameSet reads, const int32_t* klen, const uint64_t* hash, const uint64_t* table, long long nslots,
                      RgState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_name_check, dim3(wave_grid(reads.n)), dim3(RG_THREADS), 0, s, reads, klen, hash, table, nslots, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_name_probe(NameSet reads, const int32_t* klen, const uint64_t* table, long long nslots, NameSet recs, int hash_bits,
                      int32_t* read_of_record, RgState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_name_probe, dim3(wave_grid(recs.n)), dim3(RG_THREADS), 0, s, reads, klen, table, nslots, recs, hash_bits,
                       read_of_record, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_pick(const int32_t* read_of_record, const int32_t* width, long long n_records, long long n_reads,
                unsigned long long* best, int32_t* record_of_read, int32_t* records_per_read, RgState* st, hipStream_t s) {
    if (n_records > 0) {
        hipLaunchKernelGGL(k_pick_max, dim3(nblk(n_records, 256)), dim3(256), 0, s, read_of_record, width, n_records, n_reads, best,
                           records_per_read, st);
        SL_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pick_decode, dim3(nblk(n_reads, 256)), dim3(256), 0, s, best, n_reads, record_of_read);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_locus_keys(const LocusArgs& a, uint64_t* key, int32_t* idx, RgState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_locus_keys, dim3(nblk(a.n_reads, 256)), dim3(256), 0, s, a, key, idx, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_locus_ends(const LocusArgs& a, const uint64_t* skey, const int32_t* sidx, uint32_t* seg, int64_t* end, hipStream_t s) {
    hipLaunchKernelGGL(k_locus_ends, dim3(nblk(a.n_reads, 256)), dim3(256), 0, s, a, skey, sidx, seg, end);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_locus_flags(const LocusArgs& a, const uint64_t* skey, const uint32_t* seg, const int64_t* runmax, int32_t* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_locus_flags, dim3(nblk(a.n_reads + 1, 256)), dim3(256), 0, s, a, skey, seg, runmax, flag);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_locus_scatter(const LocusArgs& a, const uint64_t* skey, const int32_t* sidx, const int32_t* flag, const int32_t* before,
                         int32_t* label, RgState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_locus_scatter, dim3(nblk(a.n_reads + 1, 256)), dim3(256), 0, s, a, skey, sidx, flag, before, label, st);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_csr_keys(const int32_t* label, long long n, uint32_t* key, int32_t* member, hipStream_t s) {
    hipLaunchKernelGGL(k_csr_keys, dim3(nblk(n, 256)), dim3(256), 0, s, label, n, key, member);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_csr_heads(const uint32_t* skey, long long n, int32_t* head, hipStream_t s) {
    hipLaunchKernelGGL(k_csr_heads, dim3(nblk(n + 1, 256)), dim3(256), 0, s, skey, n, head);
    SL_HIP(hipGetLastError());
    return 0;
}

int launch_csr_offsets(const uint32_t* skey, long long n, const int32_t* head, const int32_t* before, int64_t* group_off,
                       RgState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_csr_offsets, dim3(nblk(n + 1, 256)), dim3(256), 0, s, skey, n, head, before, group_off, st);
    SL_HIP(hipGetLastError());
    return 0;
}

}  // namespace sarlacc
