// What the ingest decoders share (ecal_text.hip, ecal_raw.hip, ecal_aedat.hip, ecal_aedat4.hip, ecal_bag.hip, ecal_mcap.hip), beside
// block_utils.hpp: the clipped load and the bisection of a table's slot space, the check of a table against the file's bytes, the
// counters of a message-table ingest, the one-workgroup scan of a table, and the tails of the verdict and write kernels (their bodies:
// slot_kernels.hpp; the host driver: ingest_driver.hpp).  The load, the bisection and the table check compile for the host too
// (tests/cpp/check_ingest_blocks.cpp runs them under the sanitizers); the rest is device code (wave64; T = threads per workgroup).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ECAL_INGEST_HD __host__ __device__ __forceinline__
#define ECAL_INGEST_UNROLL _Pragma("unroll")
#else
#define ECAL_INGEST_HD inline
#define ECAL_INGEST_UNROLL
#endif

namespace ecal {

// the 32-bit word at the 4-byte aligned offset a, bytes at or behind n_bytes as zeros: nothing behind n_bytes is read
ECAL_INGEST_HD uint32_t load32_clipped(const uint8_t *__restrict__ src, uint64_t a, uint64_t n_bytes) {
    if (a + 4u <= n_bytes) return *reinterpret_cast<const uint32_t *>(src + a);
    uint32_t v = 0;
    ECAL_INGEST_UNROLL
    for (uint32_t j = 0; j < 3; j++)
        if (a + j < n_bytes) v |= (uint32_t) src[a + j] << (8u * j);
    return v;
}

// the last table entry in [lo, hi] whose first slot is not behind s (first[lo] <= s): it is not empty and holds s when
// s < first[hi + 1]
ECAL_INGEST_HD uint32_t table_find(const unsigned long long *__restrict__ first, uint32_t lo, uint32_t hi, uint64_t s) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (first[mid] <= s) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// the entries p = start, start + step, ... of a table of n that do not lie wholly within n_bytes: [offset_of(p), offset_of(p) +
// bytes_of(p)), without wrapping
template <class OffsetOf, class BytesOf>
ECAL_INGEST_HD unsigned long long table_count_outside(uint64_t n, uint64_t n_bytes, uint64_t start, uint64_t step, OffsetOf offset_of, BytesOf bytes_of) {
    unsigned long long bad = 0;
    for (uint64_t p = start; p < n; p += step) {
        const uint64_t off = offset_of(p), len = bytes_of(p);
        if (off > n_bytes || len > n_bytes - off) bad++;
    }
    return bad;
}

// the counters of one message-table ingest (device; bag and MCAP)
struct MessageWords {
    unsigned long long n_slots;      // slots of the table (MCAP EVT3: payload bytes)
    unsigned long long first_stop;   // the first slot that reaches end_time (all ones: none)
    unsigned long long n_events, n_outside, n_negative, n_before_start;
    unsigned long long bad_table;    // messages of the table that do not lie within n_bytes
};

#if defined(__HIPCC__)

// first[p] = the values of the entries before p, first[n] = all of them (returned to every thread): every thread a run of consecutive
// entries, the runs' totals scanned in the workgroup.  One workgroup of 1024 threads; one barrier, which also orders what the caller
// has stored to LDS before the call.
template <class ValueOf>
__device__ __forceinline__ unsigned long long table_exscan_1024(uint32_t n, ValueOf value_of, unsigned long long *__restrict__ first) {
    __shared__ unsigned long long s_wave[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t per = ((uint64_t) n + 1023u) / 1024u;
    const uint64_t lo = (uint64_t) threadIdx.x * per, p0 = lo < n ? lo : n, p1 = p0 + per < n ? p0 + per : n;
    unsigned long long mine = 0;
    for (uint64_t p = p0; p < p1; p++) mine += value_of(p);
    unsigned long long inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
    for (int x = 0; x < 16; x++) {
        if (x < wave) pre += s_wave[x];
        tot += s_wave[x];
    }
    unsigned long long run = pre + inc - mine;
    for (uint64_t p = p0; p < p1; p++) {
        first[p] = run;
        run += value_of(p);
    }
    if (threadIdx.x == 0) first[n] = tot;
    return tot;
}

// The tail of a verdict kernel: the block's kept count into blk_keep[blockIdx.x], and block_first() + the block's least `stop` (a slot
// within the block, 0xFFFFFFFF: none; block_first is asked by the one thread that has a stop to publish) into *first_stop by one 64-bit atomic minimum.  T / 64 pairs of LDS of its own; one barrier.
template <int T, class BlockFirst>
__device__ __forceinline__ void block_keep_and_stop(uint32_t keep, uint32_t stop, uint32_t *__restrict__ blk_keep, unsigned long long *first_stop,
                                                    BlockFirst block_first) {
    __shared__ uint32_t s_red[T / 64][2];
    const int tid = threadIdx.x;
    for (int d = 32; d > 0; d >>= 1) {
        keep += __shfl_xor(keep, d, 64);
        const uint32_t v = __shfl_xor(stop, d, 64);
        stop = v < stop ? v : stop;
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = keep;
        s_red[tid >> 6][1] = stop;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t kc = 0, sm = 0xFFFFFFFFu;
        for (int x = 0; x < T / 64; x++) {
            kc += s_red[x][0];
            sm = s_red[x][1] < sm ? s_red[x][1] : sm;
        }
        blk_keep[blockIdx.x] = kc;
        if (sm != 0xFFFFFFFFu) atomicMin(first_stop, (unsigned long long) block_first() + sm);
    }
}

// the threads' N drop counters summed in the wave and added to s_cnt[N] (LDS, zeroed in front of a barrier before this; the sums
// stand behind the next one).  Which class is which counter is the caller's.
template <int N> __device__ __forceinline__ void block_add_drops(uint32_t drop[N], uint32_t *s_cnt) {
    for (int d = 32; d > 0; d >>= 1)
        for (int i = 0; i < N; i++) drop[i] += __shfl_xor(drop[i], d, 64);
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < N; i++)
            if (drop[i]) atomicAdd(&s_cnt[i], drop[i]);
}

// The copy-out of a write kernel: the n 25-byte records staged in s_rec (LDS, complete behind a barrier) to events[at, at + n),
// clipped to the capacity: bytes up to the first 4-byte boundary of the destination, whole words, the bytes behind them.
template <int T>
__device__ __forceinline__ void block_copy_out(const uint8_t *s_rec, uint32_t n, uint8_t *__restrict__ events, uint64_t at, uint64_t capacity) {
    const int tid = threadIdx.x;
    const uint64_t room = capacity > at ? capacity - at : 0;
    const uint32_t n_out = (uint64_t) n < room ? n : (uint32_t) room;
    if (n_out) {
        uint8_t *dst = events + at * 25u;
        const uint32_t nb = n_out * 25u;
        uint32_t head = (uint32_t) ((4u - ((uintptr_t) dst & 3u)) & 3u);
        head = head < nb ? head : nb;
        const uint32_t nw = (nb - head) / 4u;
        if ((uint32_t) tid < head) dst[tid] = s_rec[tid];
        for (uint32_t j = (uint32_t) tid; j < nw; j += T) {
            const uint32_t q = head + 4u * j;
            const uint32_t v = (uint32_t) s_rec[q] | ((uint32_t) s_rec[q + 1] << 8) | ((uint32_t) s_rec[q + 2] << 16) | ((uint32_t) s_rec[q + 3] << 24);
            *reinterpret_cast<uint32_t *>(dst + q) = v;
        }
        const uint32_t tail0 = head + 4u * nw;
        if (tail0 + (uint32_t) tid < nb) dst[tail0 + tid] = s_rec[tail0 + tid];
    }
}

#endif  // __HIPCC__

}  // namespace ecal
