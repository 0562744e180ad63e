// Workgroup-level primitives shared by the kernels (wave64; T = threads per workgroup).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ecal {

// the sum of v over the workgroup, for every thread (s_red: T / 64 words, a set of its own per call; one barrier)
template <int T>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *s_red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < T / 64; w++) t += s_red[w];
    return t;
}

// the exclusive prefix of `mine` over the workgroup in thread order; *total (may be null): the workgroup's sum.  s_wsum: T / 64
// words, not to be written again before the caller's next barrier (one barrier here, behind the waves' sums)
template <int T>
__device__ __forceinline__ uint32_t block_exscan_u32(uint32_t mine, uint32_t *s_wsum, uint32_t *total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (int x = 0; x < T / 64; x++) {
        if (x < wave) pre += s_wsum[x];
        tot += s_wsum[x];
    }
    if (total) *total = tot;
    return pre + inc - mine;
}

// two independent exclusive scans of one value per thread (packed into 64 bits), totals included.
// red: >= T/64 unsigned long long of LDS.
template <int T>
__device__ __forceinline__ void block_exscan_pair(uint32_t a, uint32_t b, unsigned long long *red, uint32_t *ea,
                                                  uint32_t *eb, uint32_t *ta, uint32_t *tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long v = ((unsigned long long) b << 32) | a, inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; w++) {
        const unsigned long long x = red[w];
        if (w < wave) pre += x;
        tot += x;
    }
    __syncthreads();
    const unsigned long long ex = pre + inc - v;
    *ea = (uint32_t) ex;
    *eb = (uint32_t) (ex >> 32);
    *ta = (uint32_t) tot;
    *tb = (uint32_t) (tot >> 32);
}

// the same for two values whose totals stay below 2^16: packed into ONE 32-bit word (half the shuffles)
template <int T>
__device__ __forceinline__ void block_exscan_pair16(uint32_t a, uint32_t b, unsigned long long *red, uint32_t *ea,
                                                    uint32_t *eb, uint32_t *ta, uint32_t *tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t v = (b << 16) | a;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    uint32_t *r32 = reinterpret_cast<uint32_t *>(red);
    if (lane == 63) r32[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; w++) {
        const uint32_t x = r32[w];
        if (w < wave) pre += x;
        tot += x;
    }
    __syncthreads();
    const uint32_t ex = pre + inc - v;
    *ea = ex & 0xFFFFu;
    *eb = ex >> 16;
    *ta = tot & 0xFFFFu;
    *tb = tot >> 16;
}

// first index in [0, K] whose kf_time is not below t, by one wave: 64 probes a round (three rounds for thousands of keyframes
// where a thread's bisection takes thirteen dependent loads)
__device__ __forceinline__ uint32_t wave_lower_bound(const double *kf_time, uint32_t K, double t) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = K;   // every index below lo is < t, every index from hi on is >= t
    while (lo < hi) {
        const uint32_t span = hi - lo, step = (span + 63u) / 64u;
        const uint32_t idx = lo + lane * step;
        const bool less = idx < hi && kf_time[idx] < t;
        const uint32_t c = (uint32_t) __popcll(__ballot(less));   // ascending times: the probes below t come first
        if (c == 0) {
            hi = lo;
        } else {
            const uint32_t nhi = lo + c * step < hi ? lo + c * step : hi;
            lo = lo + (c - 1u) * step + 1u;
            hi = nhi;
        }
    }
    return lo;
}

// 16 bytes at text + off as four words, bytes at or behind n_scan as zeros: nothing behind n_scan is read
__device__ __forceinline__ uint4 load16_clipped(const uint8_t *__restrict__ text, uint64_t off, uint64_t n_scan) {
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (off + 16u <= n_scan) {
        w = *reinterpret_cast<const uint4 *>(text + off);   // (16-byte aligned: the buffer is, off is a multiple of 16)
    } else if (off < n_scan) {
        uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (off + j < n_scan) v[j >> 2] |= (uint32_t) text[off + j] << (8u * (j & 3u));
        w = make_uint4(v[0], v[1], v[2], v[3]);
    }
    return w;
}

}  // namespace ecal
