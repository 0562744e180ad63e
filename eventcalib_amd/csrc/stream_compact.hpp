// What the per-event stages of a packed 25-byte stream share on the device (ecal_activity.hip, ecal_noise.hip, ecal_undistort.hip,
// ecal_reassociate.hip): blocks of SC_BLOCK consecutive events per workgroup of SC_T threads, one verdict byte per event, the kept
// events of a block ranked in event order and written out behind the block's offset.  NO workgroup waits on another.  The arithmetic
// that decides stays with each stage; design/17_hot_pixels.md, "One copy of the filters' passes", has what was compared and measured.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "block_utils.hpp"
#include "pixel_activity.hpp"

namespace ecal {

constexpr int SC_T = 256;
constexpr uint32_t SC_BLOCK = ecal_activity::PA_BLOCK_EVENTS;
constexpr uint32_t SC_RECORD = ecal_activity::PA_RECORD_BYTES;
constexpr uint32_t SC_PER = SC_BLOCK / SC_T;        // consecutive events per thread where the verdicts are ranked
constexpr uint32_t SC_CHUNK = 1024;                 // records staged in LDS at a time (25 600 bytes)
constexpr uint32_t SC_GROUPS = SC_CHUNK / SC_PER;   // threads' runs per chunk
static_assert(SC_PER == 16, "a thread's verdicts are read as one 16-byte word, its keep bits are 16 bits");
static_assert(SC_BLOCK % SC_CHUNK == 0 && SC_CHUNK % SC_T == 0, "whole chunks, whole rounds of the workgroup");

// the events of the block that begins at event `base` (blocks of BLOCK events; base < n_events)
template <uint32_t BLOCK = SC_BLOCK>
__device__ __forceinline__ uint32_t stream_block_count(uint64_t n_events, uint64_t base) {
    return (uint32_t) (n_events - base < (uint64_t) BLOCK ? n_events - base : (uint64_t) BLOCK);
}

// The keep bits of the SC_PER events from k0 on in the block at `base`: bit e set when event k0 + e is one of the block's `count`
// and its verdict byte differs from NOT_KEPT (a template argument: as a function's it costs the filters' writing pass 19 instructions
// and 6 VGPRs).  One aligned 16-byte load (base and k0 are multiples of 16; verdict: whole blocks, the bytes behind n_events are read
// and masked); *bytes (may be null): the 16 bytes as they were read.
template <uint32_t NOT_KEPT>
__device__ __forceinline__ uint32_t verdict_keep_bits(const uint8_t *__restrict__ verdict, uint64_t base, uint32_t k0, uint32_t count,
                                                      uint4 *bytes = nullptr) {
    const uint4 w = *reinterpret_cast<const uint4 *>(verdict + base + k0);
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t e = 0; e < SC_PER; e++) {
        const uint32_t v = (words[e >> 2] >> (8u * (e & 3u))) & 0xFFu;
        bits |= (k0 + e < count && v != NOT_KEPT) ? 1u << e : 0u;
    }
    if (bytes) *bytes = w;
    return bits;
}

// The writing pass of block blockIdx.x, by all SC_T threads: reads the verdicts (16 bytes per thread), ranks the kept events inside the
// block in event order, stages their records in LDS a quarter of the block at a time — stage(r, d) puts the record at r (global) to d
// (LDS), 25 bytes — and copies them out behind out + block_off[blockIdx.x] records with aligned 16-byte stores.
// verdict: rounded up to whole blocks (the bytes behind n_events are read and masked, never written); out: room for the kept records.
template <class Stage>
__device__ __forceinline__ void compact_write_block(const uint8_t *__restrict__ rec, uint64_t n_events, const uint8_t *__restrict__ verdict,
                                                    const uint32_t *__restrict__ block_off, uint8_t *__restrict__ out, Stage stage) {
    __shared__ uint32_t s_pre[SC_T];      // the block's kept events in front of every thread's run
    __shared__ uint32_t s_bits[SC_T];     // the run's keep bits
    __shared__ uint32_t s_wsum[SC_T / 64];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[SC_CHUNK * SC_RECORD];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * SC_BLOCK;
    const uint32_t count = stream_block_count(n_events, base);
    const uint32_t bits = verdict_keep_bits<0u>(verdict, base, (uint32_t) tid * SC_PER, count);
    uint32_t ktot;
    s_pre[tid] = block_exscan_u32<SC_T>((uint32_t) __popc(bits), s_wsum, &ktot);   // (thread order = event order)
    s_bits[tid] = bits;
    __syncthreads();
    if (!ktot) return;   // (the same for every thread)
    uint8_t *const dst_blk = out + (uint64_t) block_off[blockIdx.x] * SC_RECORD;
    for (uint32_t q = 0; q * SC_CHUNK < count; q++) {
        // the kept events in front of chunk q and behind it, in the block
        const uint32_t r0 = s_pre[q * SC_GROUPS], r1 = (q + 1) * SC_CHUNK < SC_BLOCK ? s_pre[(q + 1) * SC_GROUPS] : ktot;
        if (r1 == r0) continue;   // (the same for every thread; no barrier is skipped that another thread reaches)
        // pack: lanes next to each other take events next to each other
#pragma unroll
        for (uint32_t i = 0; i < SC_CHUNK / SC_T; i++) {
            const uint32_t k = q * SC_CHUNK + i * SC_T + (uint32_t) tid, g = k / SC_PER, b = k % SC_PER;
            const uint32_t m = s_bits[g];
            if (m >> b & 1u) {   // (kept: k < count)
                const uint32_t rank = s_pre[g] + (uint32_t) __popc(m & ((1u << b) - 1u)) - r0;   // < SC_CHUNK
                stage(rec + (base + k) * SC_RECORD, s_rec + rank * SC_RECORD);
            }
        }
        __syncthreads();
        // copy-out: bytes up to the first 16-byte boundary of the destination, whole 16-byte words, the bytes behind them
        uint8_t *dst = dst_blk + (size_t) r0 * SC_RECORD;
        const uint32_t nbytes = (r1 - r0) * SC_RECORD;
        uint32_t head = (uint32_t) ((16u - ((uintptr_t) dst & 15u)) & 15u);
        head = head < nbytes ? head : nbytes;
        const uint32_t nw = (nbytes - head) / 16u;
        if ((uint32_t) tid < head) dst[tid] = s_rec[tid];
        for (uint32_t j = (uint32_t) tid; j < nw; j += SC_T) {
            const uint32_t at = head + 16u * j;
            uint4 v;
            __builtin_memcpy(&v, s_rec + at, 16);
            *reinterpret_cast<uint4 *>(dst + at) = v;
        }
        const uint32_t tail0 = head + 16u * nw;
        if (tail0 + (uint32_t) tid < nbytes) dst[tail0 + tid] = s_rec[tail0 + tid];   // (fewer than 16 bytes)
        __syncthreads();
    }
}

}  // namespace ecal
