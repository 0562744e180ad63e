// The bodies of the verdict and the write kernel of the table ingests (ecal_bag.hip, ecal_mcap.hip, ecal_aedat.hip, ecal_aedat4.hip),
// one copy each; the __global__ kernels stay in the format's file and call them.  A format is a policy F, next to its slot struct:
//   Source, Filter, Words, Slots   what the kernels are given of the file, the filter, the counters (device), the thread's slots
//   T, PER, BLOCK                  threads per workgroup, slots per thread, slots per block (wave64)
//   slots(src, s_scan)             the thread's slots; s_scan: T / 64 unsigned long long of LDS for the formats whose slots scan in the
//                                  block (AEDAT 2.0; every thread comes here)
//   is_event(slots, j)             false: a slot of no class (AEDAT 2.0's other records)
//   classify(slots, j, flt, &t, &x, &y), KEEP, STOP
//   N_DROPS, drop_class(i), drop_counter(w, i)   the classes counted, in counter order, and the field of Words each adds to
//   polarity(slots, j)             the record's polarity byte
// The slot walks and the record loads are NOT shared: they stay written out per format (design/09_measured.md, the bag ingest).
// The tails (block_keep_and_stop, block_add_drops, block_copy_out) are ingest_blocks.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include "block_utils.hpp"
#include "event_record.hpp"
#include "ingest_blocks.hpp"

namespace ecal {

// the class of every slot, the kept events per block, the first slot that reaches end_time
template <class F>
__device__ __forceinline__ void slot_verdict_body(const typename F::Source &src, const typename F::Filter &flt, uint32_t *__restrict__ blk_keep,
                                                  typename F::Words *__restrict__ w) {
    __shared__ unsigned long long s_scan[F::T / 64];
    const int tid = threadIdx.x;
    const typename F::Slots mine = F::slots(src, s_scan);
    uint32_t keep = 0, stop = 0xFFFFFFFFu;   // (stop: a slot within the block)
#pragma unroll
    for (uint32_t j = 0; j < F::PER; j++) {
        if (j < mine.n && F::is_event(mine, j)) {
            double t;
            uint32_t x, y;
            const uint8_t c = F::classify(mine, j, flt, &t, &x, &y);
            keep += c == F::KEEP ? 1u : 0u;
            const uint32_t at = (uint32_t) tid * F::PER + j;
            if (c == F::STOP && at < stop) stop = at;
        }
    }
    block_keep_and_stop<F::T>(keep, stop, blk_keep, &w->first_stop, [] { return (unsigned long long) blockIdx.x * F::BLOCK; });
}

// the kept events below the first offender, packed in LDS and copied out; the totals
template <class F>
__device__ __forceinline__ void slot_write_body(const typename F::Source &src, const uint32_t *__restrict__ blk_koff, const typename F::Filter &flt,
                                                uint8_t *__restrict__ events, uint64_t capacity, typename F::Words *__restrict__ w) {
    constexpr int T = F::T, N = F::N_DROPS;
    constexpr uint32_t PER = F::PER, BLOCK = F::BLOCK;
    __shared__ unsigned long long s_scan[T / 64];
    __shared__ uint32_t s_cnt[N];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[BLOCK * 25];
    const int tid = threadIdx.x;
    const unsigned long long X = w->first_stop;
    const uint64_t slot0 = (uint64_t) blockIdx.x * BLOCK;
    if (slot0 >= X) return;   // (the whole block lies behind the offender; the same for every thread)
    const typename F::Slots mine = F::slots(src, s_scan);
    // slots of this block below the offender: in-block slot < lim
    const uint32_t lim = X - slot0 < (unsigned long long) BLOCK ? (uint32_t) (X - slot0) : BLOCK;
    if (tid < N) s_cnt[tid] = 0;
    uint32_t keep = 0, kept_mask = 0, drop[N];
#pragma unroll
    for (int i = 0; i < N; i++) drop[i] = 0u;
    double kt[PER];
    uint32_t kx[PER], ky[PER];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        kt[j] = 0.0;
        kx[j] = ky[j] = 0u;
        if (j < mine.n && F::is_event(mine, j) && (uint32_t) tid * PER + j < lim) {
            const uint8_t c = F::classify(mine, j, flt, &kt[j], &kx[j], &ky[j]);
            if (c == F::KEEP) {
                keep++;
                kept_mask |= 1u << j;
            }
#pragma unroll
            for (int i = 0; i < N; i++) drop[i] += c == F::drop_class(i) ? 1u : 0u;
        }
    }
    uint32_t kex, eb, ktot, tb;
    block_exscan_pair<T>(keep, 0u, s_scan, &kex, &eb, &ktot, &tb);   // (its barriers order the zeroing of s_cnt too)
    block_add_drops<N>(drop, s_cnt);
    // at most BLOCK kept events: one chunk of LDS holds them all
    uint32_t k = kex;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        if (kept_mask >> j & 1u) {
            pack_record(s_rec + k * 25u, kt[j], (double) kx[j], (double) ky[j], F::polarity(mine, j));
            k++;
        }
    }
    __syncthreads();
    if (tid < N && s_cnt[tid]) atomicAdd(F::drop_counter(w, tid), (unsigned long long) s_cnt[tid]);
    if (tid == 0 && ktot) atomicAdd(&w->n_events, (unsigned long long) ktot);
    block_copy_out<T>(s_rec, ktot, events, blk_koff[blockIdx.x], capacity);
}

}  // namespace ecal
