// Raw ingest (include/ecal.h, "raw ingest"): a Prophesee EVT3 (16-bit words) or EVT2 (32-bit words) payload resident in HBM into
// packed 25-byte records.  The word step, the summary monoid and the filter are raw_events.hpp's (shared with the host decoder and
// the CPU test); design/13_raw_ingest.md has the reasoning.
//
// A block is RW_T threads x 16 bytes: 2048 EVT3 words or 1024 EVT2 words (ecal_raw_block_words).  Launches, all over 64-bit word
// offsets and with NO waiting between workgroups — state crosses blocks only between launches, or inside the one-workgroup scans:
//   1. raw_summary_kernel     one 128-bit load per thread; the summary of the thread's consecutive words, combined in the wave
//                             and in the workgroup; the block's summary and its event count (ADDR_X words + popcounts of the
//                             masked vector words — what the words emit before any drop)
//   2. ecal_scan_blocks       the blocks' first raw event index
//   3. raw_state_scan_kernel  one workgroup: the exclusive scan of the summaries with combine = every block's incoming state
//   4. raw_verdict_kernel     the block decoded from its incoming state, every event classed; the kept events per block; the raw
//                             index of the first event that reaches end_time (64-bit atomic minimum)
//   5. ecal_scan_blocks       the blocks' first kept index
//   6. raw_write_kernel       decoded again; the kept events below the first offender get their index (in-workgroup scan of the
//                             threads' counts, up to 12 a word), are packed into LDS RW_CHUNK records at a time and copied out with
//                             aligned 32-bit stores; the totals
// "The stream ends here" is the test `raw index < first offender` in pass 6: an event behind the offender may be counted as kept by
// pass 4 — that only moves offsets of blocks that pass 6 writes nothing for.
// The host sees the counters once, behind pass 6 (the file forms once more behind pass 1: the record buffer's size is a count).
// The tails of passes 4 and 6 (kept count and first offender, drop counters, copy-out) are ingest_blocks.hpp's, shared with the other
// ingests; the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <chrono>
#include <algorithm>
#include <math.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "block_utils.hpp"
#include "ingest_blocks.hpp"
#include "raw_events.hpp"

namespace ecal {

using namespace ecal_raw;

static_assert(ECAL_RAW_AUTO == RAW_FORMAT_NONE && ECAL_RAW_EVT2 == RAW_FORMAT_EVT2 && ECAL_RAW_EVT3 == RAW_FORMAT_EVT3, "format codes");

constexpr int RW_T = RAW_BLOCK_THREADS;   // threads per workgroup of the block kernels: one 128-bit load each
constexpr uint32_t RW_CHUNK = 1024;    // records staged in LDS at a time (25 600 bytes: six workgroups a CU)
constexpr unsigned long long RW_NONE = ~0ull;

template <class F> constexpr uint32_t rw_per_thread() { return 16u / F::WORD_BYTES; }
template <class F> constexpr uint32_t rw_block_words() { return raw_block_words<F>(); }

// the counters of one ingest (device)
struct RawWords {
    unsigned long long n_raw, n_other, n_wraps;
    unsigned long long first_stop;   // raw index of the first event that reaches end_time (RW_NONE: none)
    unsigned long long n_events, n_no_state, n_outside, n_negative, n_before_start;
};

// the thread's words: word j of its 16 bytes, and how many of them lie in front of n_words
template <class F> struct RwWords {
    uint64_t lo, hi;   // the 16 bytes as two register pairs: word(j) is a select and a shift
    uint32_t n;
    __device__ __forceinline__ RwWords(const uint8_t *__restrict__ payload, uint64_t n_words) {
        const uint64_t first = ((uint64_t) blockIdx.x * RW_T + threadIdx.x) * rw_per_thread<F>();
        n = first < n_words ? (uint32_t) (n_words - first < rw_per_thread<F>() ? n_words - first : rw_per_thread<F>()) : 0u;
        const uint4 q = load16_clipped(payload, first * F::WORD_BYTES, n_words * F::WORD_BYTES);
        lo = (uint64_t) q.x | ((uint64_t) q.y << 32);
        hi = (uint64_t) q.z | ((uint64_t) q.w << 32);
    }
    __device__ __forceinline__ typename F::Word word(uint32_t j) const {
        constexpr uint32_t half = rw_per_thread<F>() / 2u, bits = 8u * F::WORD_BYTES;
        return (typename F::Word) ((j < half ? lo : hi) >> (bits * (j % half)));
    }
    __device__ __forceinline__ typename F::Summary summary() const {
        typename F::Summary s = F::identity();
#pragma unroll
        for (uint32_t j = 0; j < rw_per_thread<F>(); j++)
            if (j < n) s = F::combine(s, F::of_word(word(j)));
        return s;
    }
    __device__ __forceinline__ uint32_t count() const {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < rw_per_thread<F>(); j++)
            if (j < n) c += F::count(word(j));
        return c;
    }
    // every event of the thread's words, decoded from the state `s` in front of its first word
    template <class Put> __device__ __forceinline__ void decode(typename F::Summary s, Put &&put) const {
#pragma unroll
        for (uint32_t j = 0; j < rw_per_thread<F>(); j++) {
            if (j < n) {
                const typename F::Word w = word(j);
                F::emit(s, w, put);
                s = F::combine(s, F::of_word(w));
            }
        }
    }
};

template <class S> struct RwSummaryWords {
    static_assert(sizeof(S) % 4 == 0 && alignof(S) >= 4, "summaries are 32-bit words");
    uint32_t w[sizeof(S) / 4];
};

// a summary from memory, word by word (a copy of the struct as it stands goes through scratch memory)
template <class S> __device__ __forceinline__ S rw_ld(const S *p) {
    RwSummaryWords<S> q;
#pragma unroll
    for (uint32_t i = 0; i < sizeof(S) / 4; i++) q.w[i] = reinterpret_cast<const uint32_t *>(p)[i];
    return __builtin_bit_cast(S, q);
}

template <class S> __device__ __forceinline__ S rw_shfl_up(const S &s, int d) {
    RwSummaryWords<S> q = __builtin_bit_cast(RwSummaryWords<S>, s);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(S) / 4; i++) q.w[i] = __shfl_up(q.w[i], d, 64);
    return __builtin_bit_cast(S, q);
}

// exclusive scan with F::combine of one summary per thread, thread order (combine is not commutative); *total = all of them.
// s_wave: T / 64 summaries of LDS.
template <class F, int T>
__device__ __forceinline__ void rw_block_exscan(const typename F::Summary &mine, typename F::Summary *s_wave, typename F::Summary *ex,
                                                typename F::Summary *total) {
    typedef typename F::Summary S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    S inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const S o = rw_shfl_up(inc, d);
        if (lane >= d) inc = F::combine(o, inc);
    }
    if (lane == 63) s_wave[wave] = inc;
    S prev = rw_shfl_up(inc, 1);
    if (lane == 0) prev = F::identity();
    __syncthreads();
    S pre = F::identity(), tot = F::identity();
    for (int w = 0; w < T / 64; w++) {
        const S x = rw_ld(s_wave + w);
        if (w < wave) pre = F::combine(pre, x);
        tot = F::combine(tot, x);
    }
    __syncthreads();
    *ex = F::combine(pre, prev);
    *total = tot;
}

// blk_sum / blk_cnt may be null (ecal_raw_count_events_dev wants the total alone)
template <class F>
__global__ __launch_bounds__(RW_T) void raw_summary_kernel(const uint8_t *__restrict__ payload, uint64_t n_words,
                                                           typename F::Summary *__restrict__ blk_sum, uint32_t *__restrict__ blk_cnt,
                                                           RawWords *__restrict__ w) {
    __shared__ typename F::Summary s_wave[RW_T / 64];
    __shared__ uint32_t s_red[RW_T / 64][2];
    const int tid = threadIdx.x;
    const RwWords<F> mine(payload, n_words);
    uint32_t cnt = mine.count(), other = 0;
#pragma unroll
    for (uint32_t j = 0; j < rw_per_thread<F>(); j++)
        if (j < mine.n && F::is_other(mine.word(j))) other++;
    typename F::Summary ex, total;
    rw_block_exscan<F, RW_T>(mine.summary(), s_wave, &ex, &total);
    for (int d = 32; d > 0; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
        other += __shfl_xor(other, d, 64);
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = cnt;
        s_red[tid >> 6][1] = other;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0, o = 0;
        for (int x = 0; x < RW_T / 64; x++) {
            c += s_red[x][0];
            o += s_red[x][1];
        }
        if (blk_sum) blk_sum[blockIdx.x] = total;
        if (blk_cnt) blk_cnt[blockIdx.x] = c;
        if (c) atomicAdd(&w->n_raw, (unsigned long long) c);
        if (o) atomicAdd(&w->n_other, (unsigned long long) o);
    }
}

// blk_in[b] = combine of blk_sum[0 .. b): every thread a run of consecutive blocks, the runs' totals scanned in the workgroup.
// One workgroup.
template <class F>
__global__ __launch_bounds__(1024) void raw_state_scan_kernel(const typename F::Summary *__restrict__ blk_sum, uint32_t nb,
                                                              typename F::Summary *__restrict__ blk_in, RawWords *__restrict__ w) {
    __shared__ typename F::Summary s_wave[16];
    const uint64_t per = ((uint64_t) nb + 1023u) / 1024u;
    const uint64_t lo = (uint64_t) threadIdx.x * per, b0 = lo < nb ? lo : nb, b1 = b0 + per < nb ? b0 + per : nb;
    typename F::Summary mine = F::identity();
    for (uint64_t b = b0; b < b1; b++) mine = F::combine(mine, rw_ld(blk_sum + b));
    typename F::Summary run, total;
    rw_block_exscan<F, 1024>(mine, s_wave, &run, &total);
    for (uint64_t b = b0; b < b1; b++) {
        blk_in[b] = run;
        run = F::combine(run, rw_ld(blk_sum + b));
    }
    if (threadIdx.x == 0) w->n_wraps = F::wraps(total);
}

// the class of every event, the kept events per block, the first event that reaches end_time
template <class F>
__global__ __launch_bounds__(RW_T) void raw_verdict_kernel(const uint8_t *__restrict__ payload, uint64_t n_words,
                                                           const typename F::Summary *__restrict__ blk_in, const uint32_t *__restrict__ blk_off,
                                                           RawFilter flt, uint32_t *__restrict__ blk_keep, RawWords *__restrict__ w) {
    __shared__ typename F::Summary s_wave[RW_T / 64];
    __shared__ unsigned long long s_scan[RW_T / 64];
    const RwWords<F> mine(payload, n_words);
    typename F::Summary ex, total;
    rw_block_exscan<F, RW_T>(mine.summary(), s_wave, &ex, &total);
    uint32_t raw_ex, eb, raw_tot, tb;
    block_exscan_pair<RW_T>(mine.count(), 0u, s_scan, &raw_ex, &eb, &raw_tot, &tb);
    uint32_t keep = 0, stop = 0xFFFFFFFFu, at = raw_ex;   // (indices within the block: at most 12 x 2048)
    mine.decode(F::combine(rw_ld(blk_in + blockIdx.x), ex), [&](const RawEvent &e) {
        double t;
        const uint8_t c = raw_classify(e, flt, &t);
        keep += c == RAW_CLASS_KEEP ? 1u : 0u;
        if (c == RAW_CLASS_STOP && at < stop) stop = at;
        at++;
    });
    block_keep_and_stop<RW_T>(keep, stop, blk_keep, &w->first_stop, [&] { return blk_off[blockIdx.x]; });
}

// the kept events below the first offender, packed in LDS a chunk at a time and copied out; the totals
template <class F>
__global__ __launch_bounds__(RW_T) void raw_write_kernel(const uint8_t *__restrict__ payload, uint64_t n_words,
                                                         const typename F::Summary *__restrict__ blk_in, const uint32_t *__restrict__ blk_off,
                                                         const uint32_t *__restrict__ blk_koff, RawFilter flt, uint8_t *__restrict__ events,
                                                         uint64_t capacity, RawWords *__restrict__ w) {
    __shared__ typename F::Summary s_wave[RW_T / 64];
    __shared__ unsigned long long s_scan[RW_T / 64];
    __shared__ uint32_t s_cnt[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[RW_CHUNK * 25];
    const int tid = threadIdx.x;
    const unsigned long long X = w->first_stop;
    const uint64_t raw0 = blk_off[blockIdx.x];
    if (raw0 >= X) return;   // (the whole block lies behind the offender; the same for every thread)
    const RwWords<F> mine(payload, n_words);
    typename F::Summary ex, total;
    rw_block_exscan<F, RW_T>(mine.summary(), s_wave, &ex, &total);
    const typename F::Summary state = F::combine(rw_ld(blk_in + blockIdx.x), ex);
    uint32_t raw_ex, eb, raw_tot, tb;
    block_exscan_pair<RW_T>(mine.count(), 0u, s_scan, &raw_ex, &eb, &raw_tot, &tb);
    // events of this block below the offender: in-block raw index < lim
    const uint32_t lim = X - raw0 < (unsigned long long) raw_tot ? (uint32_t) (X - raw0) : raw_tot;
    if (tid < 4) s_cnt[tid] = 0;
    uint32_t keep = 0, drop[4] = {0u, 0u, 0u, 0u}, at = raw_ex;
    mine.decode(state, [&](const RawEvent &e) {
        if (at++ < lim) {
            double t;
            const uint8_t c = raw_classify(e, flt, &t);
            keep += c == RAW_CLASS_KEEP ? 1u : 0u;
            drop[0] += c == RAW_CLASS_NO_STATE ? 1u : 0u;
            drop[1] += c == RAW_CLASS_OUTSIDE ? 1u : 0u;
            drop[2] += c == RAW_CLASS_NEGATIVE ? 1u : 0u;
            drop[3] += c == RAW_CLASS_BEFORE_START ? 1u : 0u;
        }
    });
    uint32_t kex, ktot;
    block_exscan_pair<RW_T>(keep, 0u, s_scan, &kex, &eb, &ktot, &tb);   // (its barriers order the zeroing of s_cnt too)
    block_add_drops<4>(drop, s_cnt);
    __syncthreads();
    if (tid < 4 && s_cnt[tid])
        atomicAdd(tid == 0 ? &w->n_no_state : tid == 1 ? &w->n_outside : tid == 2 ? &w->n_negative : &w->n_before_start,
                  (unsigned long long) s_cnt[tid]);
    if (tid == 0 && ktot) atomicAdd(&w->n_events, (unsigned long long) ktot);
    const uint64_t at0 = blk_koff[blockIdx.x];
    for (uint32_t c0 = 0; c0 < ktot; c0 += RW_CHUNK) {   // (ktot is the same for every thread)
        if (keep && kex < c0 + RW_CHUNK && kex + keep > c0) {
            uint32_t r = raw_ex, k = kex;
            mine.decode(state, [&](const RawEvent &e) {
                if (r++ < lim) {
                    double t;
                    if (raw_classify(e, flt, &t) == RAW_CLASS_KEEP) {
                        if (k >= c0 && k < c0 + RW_CHUNK) pack_record(s_rec + (k - c0) * 25u, t, (double) e.x, (double) e.y, e.pol);
                        k++;
                    }
                }
            });
        }
        __syncthreads();
        block_copy_out<RW_T>(s_rec, ktot - c0 < RW_CHUNK ? ktot - c0 : RW_CHUNK, events, at0 + c0, capacity);
        __syncthreads();
    }
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_raw_default_options(ecal_raw_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->format = ECAL_RAW_AUTO;
    opt->start_time = -INFINITY;
}

extern "C" uint32_t ecal_raw_block_words(int format) {
    return format == ECAL_RAW_EVT3 ? rw_block_words<Evt3>() : format == ECAL_RAW_EVT2 ? rw_block_words<Evt2>() : 0u;
}

namespace {

int raw_check_args(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, int format) {
    if (format != ECAL_RAW_EVT2 && format != ECAL_RAW_EVT3) {
        ctx->last_error = "raw ingest: no format (ECAL_RAW_EVT2 or ECAL_RAW_EVT3)";
        return ECAL_ERR_INVALID;
    }
    return ecal_ingest_check_buffer(ctx, "raw ingest", d_payload, n_bytes, 16, "payload");
}

int raw_block_count(ecal_ctx *ctx, uint64_t n_words, uint32_t block_words, uint32_t *nb) {
    const uint64_t nb64 = (n_words + block_words - 1) / block_words;
    if (nb64 > 0x7FFFFFFFull) {
        ctx->last_error = "raw ingest: the payload is too large for one launch";
        return ECAL_ERR_RANGE;
    }
    *nb = (uint32_t) nb64;
    return ECAL_OK;
}

template <class F> int raw_count(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, uint64_t *n, hipStream_t st) {
    *n = 0;
    const uint64_t n_words = n_bytes / F::WORD_BYTES;
    if (!n_words) return ECAL_OK;
    uint32_t nb = 0;
    int rc = raw_block_count(ctx, n_words, rw_block_words<F>(), &nb);
    if (rc) return rc;
    ecal_devbuf words;
    if ((rc = ecal_ensure(ctx, words, sizeof(RawWords)))) return rc;
    RawWords *d_w = words.as<RawWords>();
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(RawWords), &d_w->first_stop, st))) return rc;
    hipLaunchKernelGGL(raw_summary_kernel<F>, dim3(nb), dim3(RW_T), 0, st, d_payload, n_words, (typename F::Summary *) nullptr,
                       (uint32_t *) nullptr, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    unsigned long long raw = 0;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(&raw, &d_w->n_raw, sizeof(raw), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    *n = raw;
    return ECAL_OK;
}

// own_events != null: the records go into a buffer allocated here for the count of pass 1 (the caller's to hipFree, null when
// there is nothing to free); else into d_events / capacity
template <class F>
int raw_ingest(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_raw_options &o, uint8_t *d_events, uint64_t capacity,
               uint8_t **own_events, ecal_raw_info &I, hipStream_t st) {
    typedef typename F::Summary S;
    I.format = F::FORMAT;
    I.n_words = n_bytes / F::WORD_BYTES;
    I.n_trailing_bytes = n_bytes % F::WORD_BYTES;
    if (own_events) *own_events = nullptr;
    const uint64_t n_words = I.n_words;
    if (!n_words) return ECAL_OK;
    uint32_t nb = 0;
    int rc = raw_block_count(ctx, n_words, rw_block_words<F>(), &nb);
    if (rc) return rc;
    ecal_load_timer tm("raw", ctx->sw.load_trace, st);
    const size_t o_in = up16((size_t) nb * sizeof(S)), o_cnt = o_in + up16((size_t) nb * sizeof(S)), o_off = o_cnt + up16((size_t) nb * 4),
                 o_keep = o_off + up16(((size_t) nb + 1) * 4), o_koff = o_keep + up16((size_t) nb * 4),
                 o_words = o_koff + up16(((size_t) nb + 1) * 4), total = o_words + sizeof(RawWords);
    ecal_devbuf scratch;
    if ((rc = ecal_ensure(ctx, scratch, total))) return rc;
    uint8_t *base = scratch.as<uint8_t>();
    S *blk_sum = (S *) base, *blk_in = (S *) (base + o_in);
    uint32_t *cnt = (uint32_t *) (base + o_cnt), *off = (uint32_t *) (base + o_off), *keep = (uint32_t *) (base + o_keep),
             *koff = (uint32_t *) (base + o_koff);
    RawWords *d_w = (RawWords *) (base + o_words);
    const RawFilter flt{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time};
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(RawWords), &d_w->first_stop, st))) return rc;
    tm.mark("start");
    hipLaunchKernelGGL(raw_summary_kernel<F>, dim3(nb), dim3(RW_T), 0, st, d_payload, n_words, blk_sum, cnt, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark("summary");
    if ((rc = ecal_scan_blocks(ctx, cnt, nb, off, st))) return rc;
    hipLaunchKernelGGL(raw_state_scan_kernel<F>, dim3(1), dim3(1024), 0, st, (const S *) blk_sum, nb, blk_in, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark("block scans");
    RawWords W;
    auto fetch = [&]() { return ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st); };
    if (own_events) {   // the one count a size needs
        if ((rc = fetch())) return rc;
        if (W.n_raw > 0xFFFFFFFFull) {
            I.n_events = W.n_raw;
            ctx->last_error = "raw ingest: more than 2^32-1 events";
            return ECAL_ERR_RANGE;
        }
        capacity = W.n_raw;
        if ((rc = ecal_ingest_alloc_records(ctx, "raw ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    auto fail = [&](int code) { return ecal_ingest_drop_records(own_events, code); };
    auto launched = [&]() -> int {
        ECAL_HIP_TRY(ctx, hipGetLastError());
        return ECAL_OK;
    };
    hipLaunchKernelGGL(raw_verdict_kernel<F>, dim3(nb), dim3(RW_T), 0, st, d_payload, n_words, (const S *) blk_in, (const uint32_t *) off, flt,
                       keep, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("verdict");
    if ((rc = ecal_scan_blocks(ctx, keep, nb, koff, st))) return fail(rc);
    hipLaunchKernelGGL(raw_write_kernel<F>, dim3(nb), dim3(RW_T), 0, st, d_payload, n_words, (const S *) blk_in, (const uint32_t *) off,
                       (const uint32_t *) koff, flt, d_events, capacity, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("scan, write");
    if ((rc = fetch())) return fail(rc);
    I.n_other_words = W.n_other;
    I.n_time_wraps = W.n_wraps;
    if (W.n_raw > 0xFFFFFFFFull) {   // (the 32-bit block offsets wrapped: nothing else of this run means anything)
        I.n_events = W.n_raw;
        ctx->last_error = "raw ingest: more than 2^32-1 events";
        return fail(ECAL_ERR_RANGE);
    }
    I.n_events = W.n_events;
    I.n_no_state = W.n_no_state;
    I.n_outside = W.n_outside;
    I.n_negative = W.n_negative;
    I.n_before_start = W.n_before_start;
    I.n_after_end = W.first_stop == RW_NONE ? 0 : W.n_raw - W.first_stop;
    if (I.n_events > capacity) {
        ctx->last_error = "raw ingest: " + std::to_string(I.n_events) + " records, more than the capacity";
        return fail(ECAL_ERR_RANGE);
    }
    return ECAL_OK;
}

int raw_ingest_any(ecal_ctx *ctx, int format, const uint8_t *d_payload, uint64_t n_bytes, const ecal_raw_options &o, uint8_t *d_events,
                   uint64_t capacity, uint8_t **own_events, ecal_raw_info &I, hipStream_t st) {
    return format == ECAL_RAW_EVT3 ? raw_ingest<Evt3>(ctx, d_payload, n_bytes, o, d_events, capacity, own_events, I, st)
                                   : raw_ingest<Evt2>(ctx, d_payload, n_bytes, o, d_events, capacity, own_events, I, st);
}

// file -> header read on the host -> payload in HBM -> records in a device buffer of their own (null for none), the payload freed
int raw_file_to_events(ecal_ctx *ctx, const char *path, const ecal_raw_options *opt, uint8_t **d_events, ecal_raw_info &I) {
    *d_events = nullptr;
    ecal_raw_options o;
    if (opt) o = *opt; else ecal_raw_default_options(&o);
    if (o.format != ECAL_RAW_AUTO && o.format != ECAL_RAW_EVT2 && o.format != ECAL_RAW_EVT3) {
        ctx->last_error = "raw ingest: unknown format option";
        return ECAL_ERR_INVALID;
    }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        ctx->last_error = std::string("raw ingest: cannot open ") + path;
        return ECAL_ERR_INVALID;
    }
    // the header is a few hundred bytes of text: the first MiB of the file holds it, or it is no header of these formats
    struct stat sb;
    std::vector<uint8_t> head;
    bool ok = fstat(fd, &sb) == 0;
    if (ok) {
        head.resize((size_t) std::min<uint64_t>((uint64_t) sb.st_size, 1u << 20));
        for (size_t got = 0; ok && got < head.size();) {
            const ssize_t rd = pread(fd, head.data() + got, head.size() - got, (off_t) got);
            if (rd <= 0) ok = false;
            else got += (size_t) rd;
        }
    }
    close(fd);
    if (!ok) {
        ctx->last_error = std::string("raw ingest: cannot read ") + path;
        return ECAL_ERR_INVALID;
    }
    int header_format = ECAL_RAW_AUTO;
    uint64_t header_bytes = 0;
    if (!raw_parse_header(head.data(), head.size(), head.size() == (uint64_t) sb.st_size, &header_format, &header_bytes)) {
        ctx->last_error = std::string("raw ingest: the header does not end within the first MiB of ") + path;
        return ECAL_ERR_INVALID;
    }
    I.header_bytes = header_bytes;
    const int format = o.format != ECAL_RAW_AUTO ? o.format : header_format;
    I.format = format;
    if (format == ECAL_RAW_AUTO) {
        ctx->last_error = std::string("raw ingest: no format option and no format line in the header of ") + path;
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool trace = ctx->sw.load_trace;
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *d_payload = nullptr;
    uint64_t n_bytes = 0;
    int rc = ecal_upload_file(ctx, "raw ingest", path, header_bytes, &d_payload, &n_bytes);
    if (rc) return rc;
    if (trace)
        fprintf(stderr, "ecal raw ingest: %-24s %.3f ms\n", "file read + upload",
                1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    rc = raw_ingest_any(ctx, format, d_payload, n_bytes, o, nullptr, 0, d_events, I, ctx->stream);
    (void) hipFree(d_payload);
    return rc;
}

}  // namespace

extern "C" int ecal_raw_count_events_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, int format, uint64_t *n_events,
                                         void *stream) {
    if (!ctx || !n_events) return ECAL_ERR_INVALID;
    *n_events = 0;
    const int rc = raw_check_args(ctx, d_payload, n_bytes, format);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return format == ECAL_RAW_EVT3 ? raw_count<Evt3>(ctx, d_payload, n_bytes, n_events, (hipStream_t) stream)
                                   : raw_count<Evt2>(ctx, d_payload, n_bytes, n_events, (hipStream_t) stream);
}

extern "C" int ecal_events_from_raw_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_raw_options *opt,
                                        uint8_t *d_events, uint64_t capacity, ecal_raw_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_raw");
    if (!ctx) return ECAL_ERR_INVALID;
    ecal_raw_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    const int rc = raw_check_args(ctx, d_payload, n_bytes, opt ? opt->format : ECAL_RAW_AUTO);
    if (rc) return rc;
    if (capacity && !d_events) {
        ctx->last_error = "raw ingest: null record buffer";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int st = raw_ingest_any(ctx, opt->format, d_payload, n_bytes, *opt, d_events, capacity, nullptr, I, (hipStream_t) stream);
    if (info) *info = I;
    return st;
}

extern "C" int ecal_stream_create_from_raw_file(ecal_ctx *ctx, const char *path, const ecal_raw_options *opt, ecal_stream **out,
                                                ecal_raw_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_raw_info I;
    memset(&I, 0, sizeof(I));
    const int rc = raw_file_to_events(ctx, path, opt, &d_events, I);
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_raw_file", d_events, I.n_events, out);
}

extern "C" int ecal_raw_to_bin_file(ecal_ctx *ctx, const char *raw_path, const char *bin_path, const ecal_raw_options *opt,
                                    ecal_raw_info *info) {
    if (!ctx || !raw_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_raw_info I;
    memset(&I, 0, sizeof(I));
    const int rc = raw_file_to_events(ctx, raw_path, opt, &d_events, I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_raw_to_bin_file", d_events, I.n_events, bin_path);
}
