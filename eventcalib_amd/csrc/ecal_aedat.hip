// AEDAT ingest (include/ecal.h, "aedat ingest"): an iniVation AEDAT 3.1 or 2.0 payload resident in HBM into packed 25-byte records.
// The field extraction, the wrap flag, the filter, the header parser and the packet indexer are aedat_events.hpp's (shared with the
// host decoder and the CPU test); design/15_aedat_ingest.md has the reasoning.
//
// The 3.1 packet chain is NOT walked here: a packet is found only through the header before it, one dependent 28-byte load a
// packet.  The host indexes the polarity packets (ecal_aedat_index_packets) and the table comes in with the payload.
//
// A block is AE_T threads x 4 consecutive slots = 1024 slots (ecal_aedat_block_events).  A slot is an event of the table's slot
// space (3.1) or an 8-byte record (2.0; a record that is no DVS event is a slot of no class).  Launches, with NO waiting between
// workgroups — state crosses blocks only between launches, or inside the one-workgroup scans:
//   3.1  1. aedat_packet_scan_kernel  one workgroup: the exclusive 64-bit scan of the table's n_events = every packet's first slot;
//                                     the table checked against n_bytes
//   2.0  1. aedat20_count_kernel      wrap flags and DVS events per block (a thread's first record reads its predecessor's stamp)
//        2. ecal_scan_blocks          the wraps in front of every block
//   both 3. aedat_verdict_kernel      every slot classed; the kept events per block; the first slot that reaches end_time (64-bit
//                                     atomic minimum)
//        4. ecal_scan_blocks          the blocks' first kept index
//        5. aedat_write_kernel        classed again; the kept events below the first offender get their index (in-workgroup scan),
//                                     are packed into LDS and copied out with aligned 32-bit stores; the totals
// "The stream ends here" is the test `slot < first offender` in pass 5, as in the raw ingest.  The host sees the counters once,
// behind pass 5 (the file forms of 2.0 once more behind pass 1: the record buffer's size is a count).
// The table scan, the bisection, the clipped load and the tails of passes 3 and 5 are ingest_blocks.hpp's, shared with the other
// ingests; the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "block_utils.hpp"
#include "ingest_blocks.hpp"
#include "aedat_events.hpp"

namespace ecal {

using namespace ecal_aedat;

static_assert(ECAL_AEDAT_AUTO == AEDAT_FORMAT_NONE && ECAL_AEDAT_2_0 == AEDAT_FORMAT_20 && ECAL_AEDAT_3_1 == AEDAT_FORMAT_31, "format codes");
static_assert(ECAL_ERR_INVALID == AEDAT_INVALID && ECAL_ERR_RANGE == AEDAT_RANGE && ECAL_OK == AEDAT_OK, "status codes");
static_assert(sizeof(ecal_aedat_packet) == 16 && sizeof(AedatPacket) == 16, "packet table entry");

constexpr int AE_T = AEDAT_BLOCK_THREADS;
constexpr uint32_t AE_PER = AEDAT_THREAD_EVENTS;
constexpr uint32_t AE_BLOCK = AEDAT_BLOCK_EVENTS;   // slots per block, and records staged in LDS (25 600 bytes: six workgroups a CU)
constexpr unsigned long long AE_NONE = ~0ull;

// the counters of one ingest (device)
struct AedatWords {
    unsigned long long n_slots;      // 3.1: slots of the table
    unsigned long long n_dvs;        // 2.0: DVS records
    unsigned long long n_other;      // 2.0: the other records
    unsigned long long first_stop;   // the first slot that reaches end_time (AE_NONE: none)
    unsigned long long n_events, n_invalid, n_outside, n_negative, n_before_start;
    unsigned long long bad_table;    // 3.1: packets of the table that do not lie within n_bytes
};

// what a block kernel is given of the payload
struct AedatSource {
    const uint8_t *payload;
    uint64_t n_bytes;
    uint64_t n_slots;                       // slots in all
    const AedatPacket *packets;             // 3.1
    const unsigned long long *first;        // 3.1: [n_packets + 1]
    uint32_t n_packets;
    const uint32_t *blk_wraps_in;           // 2.0: wraps in front of every block
};

// The thread's slots: three words a slot.  3.1: data, stamp, the packet's overflow.  2.0: address, stamp, the wraps up to and
// including the record (both words swapped to host order).
template <int FMT> struct AeSlots {
    uint32_t a[AE_PER], ts[AE_PER], hi[AE_PER];
    uint32_t n;      // slots of this thread in front of n_slots
    uint32_t flags;  // 2.0: the wrap flags of the thread's records, summed

    // s_scan: AE_T / 64 unsigned long long of LDS (2.0 with wraps: the in-block scan of the flags; every thread must come here)
    __device__ __forceinline__ AeSlots(const AedatSource &src, unsigned long long *s_scan, bool with_wraps) {
        const uint64_t s0 = ((uint64_t) blockIdx.x * AE_T + threadIdx.x) * AE_PER;
        n = s0 < src.n_slots ? (uint32_t) (src.n_slots - s0 < AE_PER ? src.n_slots - s0 : AE_PER) : 0u;
        flags = 0;
        if constexpr (FMT == AEDAT_FORMAT_31) {
            (void) s_scan; (void) with_wraps;
#pragma unroll
            for (uint32_t j = 0; j < AE_PER; j++) a[j] = ts[j] = hi[j] = 0u;
            if (n) {
                // the block's packets by bisection (the same for every thread), the thread's inside them
                const uint64_t b0 = (uint64_t) blockIdx.x * AE_BLOCK;
                const uint64_t b1 = b0 + AE_BLOCK < src.n_slots ? b0 + AE_BLOCK - 1u : src.n_slots - 1u;
                const uint32_t p_lo = table_find(src.first, 0u, src.n_packets - 1u, b0);
                const uint32_t p_hi = table_find(src.first, p_lo, src.n_packets - 1u, b1);
                uint32_t p = table_find(src.first, p_lo, p_hi, s0);
                uint64_t p_first = src.first[p], p_next = src.first[p + 1], p_off = src.packets[p].offset;
                uint32_t p_ovf = (uint32_t) src.packets[p].ts_overflow;
#pragma unroll
                for (uint32_t j = 0; j < AE_PER; j++) {
                    if (j < n) {
                        const uint64_t s = s0 + j;
                        if (s >= p_next) {   // (packets of no events in between are stepped over by the search)
                            p = table_find(src.first, p + 1u, p_hi, s);
                            p_first = src.first[p];
                            p_next = src.first[p + 1];
                            p_off = src.packets[p].offset;
                            p_ovf = (uint32_t) src.packets[p].ts_overflow;
                        }
                        // the record from aligned words, whatever its byte offset; a table that points behind the payload
                        // (bad_table, an error on the host) reads zeros
                        const uint64_t off = p_off + (s - p_first) * 8u;
                        if (off + 8u <= src.n_bytes && off + 8u > off) {
                            const uint64_t al = off & ~3ull;
                            const uint32_t sh = 8u * (uint32_t) (off & 3u);
                            const uint32_t w0 = *reinterpret_cast<const uint32_t *>(src.payload + al);
                            const uint32_t w1 = *reinterpret_cast<const uint32_t *>(src.payload + al + 4u);
                            const uint32_t w2 = sh ? load32_clipped(src.payload, al + 8u, src.n_bytes) : 0u;
                            a[j] = (uint32_t) ((((uint64_t) w1 << 32) | w0) >> sh);
                            ts[j] = (uint32_t) ((((uint64_t) w2 << 32) | w1) >> sh);
                        }
                        hi[j] = p_ovf;
                    }
                }
            }
        } else {
            // 32 bytes at a multiple of 32: two aligned 128-bit loads, clipped to the whole records
            const uint64_t n_scan = src.n_slots * 8u;
            const uint4 q0 = load16_clipped(src.payload, s0 * 8u, n_scan), q1 = load16_clipped(src.payload, s0 * 8u + 16u, n_scan);
            a[0] = __builtin_bswap32(q0.x); ts[0] = __builtin_bswap32(q0.y);
            a[1] = __builtin_bswap32(q0.z); ts[1] = __builtin_bswap32(q0.w);
            a[2] = __builtin_bswap32(q1.x); ts[2] = __builtin_bswap32(q1.y);
            a[3] = __builtin_bswap32(q1.z); ts[3] = __builtin_bswap32(q1.w);
            uint32_t prev = 0;
            if (n && s0) prev = __builtin_bswap32(*reinterpret_cast<const uint32_t *>(src.payload + s0 * 8u - 4u));
#pragma unroll
            for (uint32_t j = 0; j < AE_PER; j++) {
                if (j < n && (s0 || j)) flags += aedat20_wrap(prev, ts[j]);
                hi[j] = flags;   // (inclusive, within the thread)
                prev = ts[j];
            }
            if (with_wraps) {
                uint32_t ex, eb, tot, tb;
                block_exscan_pair<AE_T>(flags, 0u, s_scan, &ex, &eb, &tot, &tb);
                const uint32_t base = src.blk_wraps_in[blockIdx.x] + ex;
#pragma unroll
                for (uint32_t j = 0; j < AE_PER; j++) hi[j] += base;
            }
        }
    }
    __device__ __forceinline__ bool is_event(uint32_t j) const {
        if constexpr (FMT == AEDAT_FORMAT_31) return true;
        else return aedat20_is_event(a[j]);
    }
    __device__ __forceinline__ AedatEvent event(uint32_t j) const {
        if constexpr (FMT == AEDAT_FORMAT_31) return aedat31_event(a[j], ts[j], (int32_t) hi[j]);
        else return aedat20_event(a[j], ts[j], (uint64_t) hi[j]);
    }
};

// first[p] = n_events of the packets before p, first[n] = all of them (table_exscan_1024); the table checked against n_bytes.
// One workgroup.
__global__ __launch_bounds__(1024) void aedat_packet_scan_kernel(const AedatPacket *__restrict__ packets, uint32_t n, uint64_t n_bytes,
                                                                 unsigned long long *__restrict__ first, AedatWords *__restrict__ w) {
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (unsigned long long) packets[p].n_events; }, first);
    if (threadIdx.x == 0) w->n_slots = tot;
    // (a pass of its own, strided: the table is read once more than the scan needs; the scan's value_of runs twice an entry)
    unsigned long long bad = 0;
    for (uint64_t p = threadIdx.x; p < n; p += 1024u) {
        const uint64_t off = packets[p].offset, len = (uint64_t) packets[p].n_events * 8u;
        if (off > n_bytes || len > n_bytes - off) bad++;
    }
    if (bad) atomicAdd(&w->bad_table, bad);
}

// 2.0: the block's wrap flags and its DVS / other records
__global__ __launch_bounds__(AE_T) void aedat20_count_kernel(AedatSource src, uint32_t *__restrict__ blk_wraps, AedatWords *__restrict__ w) {
    __shared__ uint32_t s_red[AE_T / 64][3];
    const int tid = threadIdx.x;
    const AeSlots<AEDAT_FORMAT_20> mine(src, nullptr, false);
    uint32_t wraps = mine.flags, dvs = 0, other = 0;
#pragma unroll
    for (uint32_t j = 0; j < AE_PER; j++) {
        if (j < mine.n) {
            if (mine.is_event(j)) dvs++; else other++;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        wraps += __shfl_xor(wraps, d, 64);
        dvs += __shfl_xor(dvs, d, 64);
        other += __shfl_xor(other, d, 64);
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = wraps;
        s_red[tid >> 6][1] = dvs;
        s_red[tid >> 6][2] = other;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0, e = 0, o = 0;
        for (int x = 0; x < AE_T / 64; x++) {
            c += s_red[x][0];
            e += s_red[x][1];
            o += s_red[x][2];
        }
        if (blk_wraps) blk_wraps[blockIdx.x] = c;
        if (e) atomicAdd(&w->n_dvs, (unsigned long long) e);
        if (o) atomicAdd(&w->n_other, (unsigned long long) o);
    }
}

// the class of every slot, the kept events per block, the first slot that reaches end_time
template <int FMT>
__global__ __launch_bounds__(AE_T) void aedat_verdict_kernel(AedatSource src, AedatFilter flt, uint32_t *__restrict__ blk_keep,
                                                             AedatWords *__restrict__ w) {
    __shared__ unsigned long long s_scan[AE_T / 64];
    const int tid = threadIdx.x;
    const AeSlots<FMT> mine(src, s_scan, true);
    uint32_t keep = 0, stop = 0xFFFFFFFFu;   // (stop: a slot within the block)
#pragma unroll
    for (uint32_t j = 0; j < AE_PER; j++) {
        if (j < mine.n && mine.is_event(j)) {
            double t;
            uint32_t x, y;
            const uint8_t c = aedat_classify(mine.event(j), flt, &t, &x, &y);
            keep += c == AEDAT_CLASS_KEEP ? 1u : 0u;
            const uint32_t at = (uint32_t) tid * AE_PER + j;
            if (c == AEDAT_CLASS_STOP && at < stop) stop = at;
        }
    }
    block_keep_and_stop<AE_T>(keep, stop, blk_keep, &w->first_stop, [] { return (unsigned long long) blockIdx.x * AE_BLOCK; });
}

// the kept events below the first offender, packed in LDS and copied out; the totals
template <int FMT>
__global__ __launch_bounds__(AE_T) void aedat_write_kernel(AedatSource src, const uint32_t *__restrict__ blk_koff, AedatFilter flt,
                                                           uint8_t *__restrict__ events, uint64_t capacity, AedatWords *__restrict__ w) {
    __shared__ unsigned long long s_scan[AE_T / 64];
    __shared__ uint32_t s_cnt[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[AE_BLOCK * 25];
    const int tid = threadIdx.x;
    const unsigned long long X = w->first_stop;
    const uint64_t slot0 = (uint64_t) blockIdx.x * AE_BLOCK;
    if (slot0 >= X) return;   // (the whole block lies behind the offender; the same for every thread)
    const AeSlots<FMT> mine(src, s_scan, true);
    // slots of this block below the offender: in-block slot < lim
    const uint32_t lim = X - slot0 < (unsigned long long) AE_BLOCK ? (uint32_t) (X - slot0) : AE_BLOCK;
    if (tid < 4) s_cnt[tid] = 0;
    uint32_t keep = 0, kept_mask = 0, drop[4] = {0u, 0u, 0u, 0u};
    double kt[AE_PER];
    uint32_t kx[AE_PER], ky[AE_PER];
#pragma unroll
    for (uint32_t j = 0; j < AE_PER; j++) {
        kt[j] = 0.0;
        kx[j] = ky[j] = 0u;
        if (j < mine.n && mine.is_event(j) && (uint32_t) tid * AE_PER + j < lim) {
            const uint8_t c = aedat_classify(mine.event(j), flt, &kt[j], &kx[j], &ky[j]);
            if (c == AEDAT_CLASS_KEEP) {
                keep++;
                kept_mask |= 1u << j;
            }
            drop[0] += c == AEDAT_CLASS_INVALID ? 1u : 0u;
            drop[1] += c == AEDAT_CLASS_OUTSIDE ? 1u : 0u;
            drop[2] += c == AEDAT_CLASS_NEGATIVE ? 1u : 0u;
            drop[3] += c == AEDAT_CLASS_BEFORE_START ? 1u : 0u;
        }
    }
    uint32_t kex, eb, ktot, tb;
    block_exscan_pair<AE_T>(keep, 0u, s_scan, &kex, &eb, &ktot, &tb);   // (its barriers order the zeroing of s_cnt too)
    block_add_drops<4>(drop, s_cnt);
    // at most AE_BLOCK kept events: one chunk of LDS holds them all
    uint32_t k = kex;
#pragma unroll
    for (uint32_t j = 0; j < AE_PER; j++) {
        if (kept_mask >> j & 1u) {
            pack_record(s_rec + k * 25u, kt[j], (double) kx[j], (double) ky[j],
                        (uint8_t) (FMT == AEDAT_FORMAT_31 ? (mine.a[j] >> 1) & 1u : (mine.a[j] >> 11) & 1u));
            k++;
        }
    }
    __syncthreads();
    if (tid < 4 && s_cnt[tid])
        atomicAdd(tid == 0 ? &w->n_invalid : tid == 1 ? &w->n_outside : tid == 2 ? &w->n_negative : &w->n_before_start,
                  (unsigned long long) s_cnt[tid]);
    if (tid == 0 && ktot) atomicAdd(&w->n_events, (unsigned long long) ktot);
    block_copy_out<AE_T>(s_rec, ktot, events, blk_koff[blockIdx.x], capacity);
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_aedat_default_options(ecal_aedat_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->format = ECAL_AEDAT_AUTO;
    opt->source = -1;
    opt->start_time = -INFINITY;
}

extern "C" uint32_t ecal_aedat_block_events(int format) {
    return format == ECAL_AEDAT_3_1 || format == ECAL_AEDAT_2_0 ? AE_BLOCK : 0u;
}

namespace {

void aedat_info_from_counts(ecal_aedat_info &I, const AedatCounts &c) {
    I.n_raw_events = c.n_raw_events;
    I.n_packets = c.n_packets;
    I.n_other_packets = c.n_other_packets;
    I.n_trailing_bytes = c.n_trailing_bytes;
}

int aedat_check_args(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const void *d_packets, uint64_t n_packets, int format) {
    if (format != ECAL_AEDAT_2_0 && format != ECAL_AEDAT_3_1) {
        ctx->last_error = "aedat ingest: no format (ECAL_AEDAT_3_1 or ECAL_AEDAT_2_0)";
        return ECAL_ERR_INVALID;
    }
    int rc = ecal_ingest_check_buffer(ctx, "aedat ingest", d_payload, n_bytes, 16, "payload");
    if (!rc && format == ECAL_AEDAT_3_1) rc = ecal_ingest_check_buffer(ctx, "aedat ingest", d_packets, n_packets, 8, "packet table", nullptr, "packets");
    return rc;
}

int aedat_check_options(ecal_ctx *ctx, const ecal_aedat_options &o) {
    if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) {
        ctx->last_error = "aedat ingest: flip_x / flip_y need width / height";
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

// n_slots_host: 3.1, the sum of the table's n_events when the caller knows it (the file forms), else AE_NONE.
// own_events != null: the records go into a buffer allocated here for the count (the caller's to hipFree, null when there is
// nothing to free); else into d_events / capacity
template <int FMT>
int aedat_ingest(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const AedatPacket *d_packets, uint64_t n_packets,
                 uint64_t n_slots_host, const ecal_aedat_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events,
                 ecal_aedat_info &I, hipStream_t st) {
    constexpr bool V31 = FMT == AEDAT_FORMAT_31;
    I.format = FMT;
    if (own_events) *own_events = nullptr;
    uint64_t bound;   // no fewer than the slots: sizes the per-block arrays
    if (V31) {
        I.n_packets = n_packets;
        if (!n_packets || n_slots_host == 0) return ECAL_OK;
        bound = n_slots_host != AE_NONE ? n_slots_host : std::min<uint64_t>(n_bytes / 8u, 0xFFFFFFFFull);
    } else {
        I.n_records = n_bytes / 8u;
        I.n_trailing_bytes = n_bytes % 8u;
        bound = I.n_records;
        if (!bound) return ECAL_OK;
    }
    if (bound > 0xFFFFFFFFull) {
        I.n_events = bound;
        ctx->last_error = "aedat ingest: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    const uint32_t nb_max = (uint32_t) ((bound + AE_BLOCK - 1) / AE_BLOCK);
    ecal_load_timer tm("aedat", ctx->sw.load_trace, st);
    const size_t o_first = 0, o_wr = o_first + up16((size_t) (V31 ? n_packets + 1 : 0) * 8), o_win = o_wr + up16((size_t) nb_max * 4),
                 o_keep = o_win + up16(((size_t) nb_max + 1) * 4), o_koff = o_keep + up16((size_t) nb_max * 4),
                 o_words = o_koff + up16(((size_t) nb_max + 1) * 4), total = o_words + sizeof(AedatWords);
    ecal_devbuf scratch;
    int rc;
    if ((rc = ecal_ensure(ctx, scratch, total))) return rc;
    uint8_t *base = scratch.as<uint8_t>();
    unsigned long long *first = (unsigned long long *) (base + o_first);
    uint32_t *wr = (uint32_t *) (base + o_wr), *win = (uint32_t *) (base + o_win), *keep = (uint32_t *) (base + o_keep),
             *koff = (uint32_t *) (base + o_koff);
    AedatWords *d_w = (AedatWords *) (base + o_words);
    const AedatFilter flt{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(AedatWords), &d_w->first_stop, st))) return rc;
    tm.mark("start");
    AedatSource src{d_payload, n_bytes, bound, d_packets, first, (uint32_t) n_packets, win};
    AedatWords W;
    auto fetch = [&]() { return ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st); };
    uint32_t nb = nb_max;
    if (V31) {
        hipLaunchKernelGGL(aedat_packet_scan_kernel, dim3(1), dim3(1024), 0, st, d_packets, (uint32_t) n_packets, n_bytes, first, d_w);
        ECAL_HIP_TRY(ctx, hipGetLastError());
        tm.mark("packet scan");
        if (n_slots_host == AE_NONE) {   // the grid is a count of the table: one look at it
            if ((rc = fetch())) return rc;
            if (W.bad_table) {
                ctx->last_error = "aedat ingest: " + std::to_string(W.bad_table) + " packets of the table do not lie within the payload";
                return ECAL_ERR_INVALID;
            }
            if (W.n_slots > 0xFFFFFFFFull) {
                I.n_events = W.n_slots;
                ctx->last_error = "aedat ingest: more than 2^32-1 events";
                return ECAL_ERR_RANGE;
            }
            if (W.n_slots > bound) {   // (packets that overlap: more events than the payload has room for)
                ctx->last_error = "aedat ingest: the packet table names more events than the payload holds";
                return ECAL_ERR_INVALID;
            }
            src.n_slots = W.n_slots;
            nb = (uint32_t) ((W.n_slots + AE_BLOCK - 1) / AE_BLOCK);
        }
        I.n_raw_events = src.n_slots;
        if (!src.n_slots) return ECAL_OK;
        if (own_events) capacity = src.n_slots;
    } else {
        hipLaunchKernelGGL(aedat20_count_kernel, dim3(nb), dim3(AE_T), 0, st, src, wr, d_w);
        ECAL_HIP_TRY(ctx, hipGetLastError());
        tm.mark("wrap count");
        if ((rc = ecal_scan_blocks(ctx, wr, nb, win, st))) return rc;
        tm.mark("wrap scan");
        if (own_events) {   // the one count a size needs
            if ((rc = fetch())) return rc;
            capacity = W.n_dvs;
        }
    }
    if (own_events) {
        if ((rc = ecal_ingest_alloc_records(ctx, "aedat ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    auto fail = [&](int code) { return ecal_ingest_drop_records(own_events, code); };
    auto launched = [&]() -> int {
        ECAL_HIP_TRY(ctx, hipGetLastError());
        return ECAL_OK;
    };
    hipLaunchKernelGGL(aedat_verdict_kernel<FMT>, dim3(nb), dim3(AE_T), 0, st, src, flt, keep, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("verdict");
    if ((rc = ecal_scan_blocks(ctx, keep, nb, koff, st))) return fail(rc);
    hipLaunchKernelGGL(aedat_write_kernel<FMT>, dim3(nb), dim3(AE_T), 0, st, src, (const uint32_t *) koff, flt, d_events, capacity, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("scan, write");
    if ((rc = fetch())) return fail(rc);
    if (V31) {
        if (W.bad_table || W.n_slots != src.n_slots) {
            ctx->last_error = "aedat ingest: the packet table does not fit the payload (" + std::to_string(W.bad_table) +
                              " packets outside it, " + std::to_string(W.n_slots) + " events)";
            return fail(ECAL_ERR_INVALID);
        }
    } else {
        I.n_other_records = W.n_other;
        I.n_raw_events = W.n_dvs;
        uint32_t wraps = 0;   // (the scan's total stands behind the blocks' offsets)
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(&wraps, win + nb, 4, hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
        I.n_time_wraps = wraps;
    }
    I.n_events = W.n_events;
    I.n_invalid = W.n_invalid;
    I.n_outside = W.n_outside;
    I.n_negative = W.n_negative;
    I.n_before_start = W.n_before_start;
    // every event in front of the offender has one of the five classes
    I.n_after_end = W.first_stop == AE_NONE ? 0 : I.n_raw_events - (W.n_events + W.n_invalid + W.n_outside + W.n_negative + W.n_before_start);
    if (I.n_events > capacity) {
        ctx->last_error = "aedat ingest: " + std::to_string(I.n_events) + " records, more than the capacity";
        return fail(ECAL_ERR_RANGE);
    }
    return ECAL_OK;
}

int aedat_ingest_any(ecal_ctx *ctx, int format, const uint8_t *d_payload, uint64_t n_bytes, const AedatPacket *d_packets, uint64_t n_packets,
                     uint64_t n_slots_host, const ecal_aedat_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events,
                     ecal_aedat_info &I, hipStream_t st) {
    return format == ECAL_AEDAT_3_1
               ? aedat_ingest<AEDAT_FORMAT_31>(ctx, d_payload, n_bytes, d_packets, n_packets, n_slots_host, o, d_events, capacity, own_events, I, st)
               : aedat_ingest<AEDAT_FORMAT_20>(ctx, d_payload, n_bytes, nullptr, 0, AE_NONE, o, d_events, capacity, own_events, I, st);
}

bool aedat_pread(int fd, void *dst, size_t n, uint64_t at) {
    for (size_t got = 0; got < n;) {
        const ssize_t rd = pread(fd, (uint8_t *) dst + got, n - got, (off_t) (at + got));
        if (rd <= 0) return false;
        got += (size_t) rd;
    }
    return true;
}

// The packet table of a 3.1 file: the headers alone are read, one pread of 28 bytes a packet at the place the one before names (a
// sparse second read of a file whose bytes pass through host memory anyway).  That is a system call a packet — milliseconds for
// 50 M events, where the walk over memory takes a tenth of one (design/09_measured.md; a memory map, a page fault a packet, and
// windows of the file around every header were several times slower still) — so the caller runs this on a thread of its own
// beside the upload: nothing of the context is touched here, *error takes the text.
int aedat_index_file(int fd, uint64_t header_bytes, uint64_t file_bytes, int source, std::vector<AedatPacket> &table, AedatCounts &c,
                     const char *path, std::string *error) {
    memset(&c, 0, sizeof(c));
    if (file_bytes <= header_bytes) return ECAL_OK;
    std::string err;
    const int rc = aedat31_walk_headers(
        [&](uint64_t pos, uint8_t *raw) { return aedat_pread(fd, raw, AEDAT31_HEADER_BYTES, header_bytes + pos); }, file_bytes - header_bytes,
        source, c, [&](const AedatPacket &p) { table.push_back(p); }, &err);
    if (rc) *error = "aedat ingest: " + err + " (" + path + ")";
    return rc;
}

// file -> header read on the host -> (3.1: packets indexed on the host, beside the upload) -> payload in HBM -> records in a device buffer of their own
// (null for none), the payload freed
int aedat_file_to_events(ecal_ctx *ctx, const char *path, const ecal_aedat_options *opt, uint8_t **d_events, ecal_aedat_info &I) {
    *d_events = nullptr;
    ecal_aedat_options o;
    if (opt) o = *opt; else ecal_aedat_default_options(&o);
    if (o.format != ECAL_AEDAT_AUTO && o.format != ECAL_AEDAT_2_0 && o.format != ECAL_AEDAT_3_1) {
        ctx->last_error = "aedat ingest: unknown format option";
        return ECAL_ERR_INVALID;
    }
    int rc = aedat_check_options(ctx, o);
    if (rc) return rc;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        ctx->last_error = std::string("aedat ingest: cannot open ") + path;
        return ECAL_ERR_INVALID;
    }
    struct stat sb;
    std::vector<uint8_t> head;
    bool ok = fstat(fd, &sb) == 0;
    if (ok) {
        head.resize((size_t) std::min<uint64_t>((uint64_t) sb.st_size, 1u << 20));
        ok = aedat_pread(fd, head.data(), head.size(), 0);
    }
    if (!ok) {
        close(fd);
        ctx->last_error = std::string("aedat ingest: cannot read ") + path;
        return ECAL_ERR_INVALID;
    }
    int format = ECAL_AEDAT_AUTO;
    uint64_t header_bytes = 0;
    std::string err;
    if (aedat_parse_header(head.data(), head.size(), head.size() == (uint64_t) sb.st_size, o.format, &format, &header_bytes, &err)) {
        close(fd);
        ctx->last_error = "aedat ingest: " + err + " (" + path + ")";
        return ECAL_ERR_INVALID;
    }
    I.header_bytes = header_bytes;
    I.format = format;
    std::vector<AedatPacket> table;
    AedatCounts c;
    memset(&c, 0, sizeof(c));
    ecal_ingest_index_fn index;   // (2.0 has no packets to index)
    if (format == ECAL_AEDAT_3_1)
        index = [&](std::string *error, const void **tab, size_t *tab_bytes) {
            const int index_rc = aedat_index_file(fd, header_bytes, (uint64_t) sb.st_size, o.source, table, c, path, error);
            *tab = table.data();
            *tab_bytes = table.size() * sizeof(AedatPacket);
            return index_rc;
        };
    ecal_ingest_upload up;
    if ((rc = ecal_ingest_upload_indexed(ctx, "aedat", "aedat ingest", "host packet index", path, fd, header_bytes, ECAL_INGEST_ANY_SIZE, index, &up))) return rc;
    aedat_info_from_counts(I, c);
    const uint64_t trailing = I.n_trailing_bytes;
    rc = aedat_ingest_any(ctx, format, up.d_file, up.n_bytes, (const AedatPacket *) up.d_table, table.size(), c.n_raw_events, o, nullptr, 0, d_events, I,
                          ctx->stream);
    if (format == ECAL_AEDAT_3_1) I.n_trailing_bytes = trailing;
    ecal_ingest_free_upload(ctx, &up);
    return rc;
}

}  // namespace

extern "C" int ecal_aedat_parse_header(ecal_ctx *ctx, const uint8_t *data, uint64_t n_bytes, int *format, uint64_t *header_bytes) {
    if (!format || !header_bytes || (n_bytes && !data)) return ECAL_ERR_INVALID;
    std::string err;
    const int rc = aedat_parse_header(data, (size_t) n_bytes, true, *format, format, header_bytes, &err);
    if (rc && ctx) ctx->last_error = "ecal_aedat_parse_header: " + err;
    return rc;
}

extern "C" int ecal_aedat_index_packets(ecal_ctx *ctx, const uint8_t *payload_host, uint64_t n_bytes, int source, ecal_aedat_packet *out,
                                        uint64_t capacity, uint64_t *n_packets, ecal_aedat_info *info) {
    if (!n_packets || (n_bytes && !payload_host) || (capacity && !out)) return ECAL_ERR_INVALID;
    AedatCounts c;
    memset(&c, 0, sizeof(c));
    std::string err;
    const int rc = aedat_index_packets(payload_host, n_bytes, source, reinterpret_cast<AedatPacket *>(out), capacity, n_packets, c, &err);
    if (rc && ctx) ctx->last_error = "ecal_aedat_index_packets: " + err;
    if (info && rc != ECAL_ERR_INVALID) {
        memset(info, 0, sizeof(*info));
        info->format = ECAL_AEDAT_3_1;
        aedat_info_from_counts(*info, c);
    }
    return rc;
}

extern "C" int ecal_aedat_count_events_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_aedat_packet *d_packets,
                                           uint64_t n_packets, int format, uint64_t *n_events, void *stream) {
    if (!ctx || !n_events) return ECAL_ERR_INVALID;
    *n_events = 0;
    int rc = aedat_check_args(ctx, d_payload, n_bytes, d_packets, n_packets, format);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    const bool v31 = format == ECAL_AEDAT_3_1;
    const uint64_t n_rec = n_bytes / 8u;
    if (v31 ? !n_packets : !n_rec) return ECAL_OK;
    if (!v31 && n_rec > 0xFFFFFFFFull) {
        ctx->last_error = "aedat ingest: more than 2^32-1 records";
        return ECAL_ERR_RANGE;
    }
    ecal_devbuf buf;
    const size_t o_words = up16((size_t) (v31 ? n_packets + 1 : 0) * 8);
    if ((rc = ecal_ensure(ctx, buf, o_words + sizeof(AedatWords)))) return rc;
    AedatWords *d_w = (AedatWords *) (buf.as<uint8_t>() + o_words);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(AedatWords), &d_w->first_stop, st))) return rc;
    if (v31) {
        hipLaunchKernelGGL(aedat_packet_scan_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<const AedatPacket *>(d_packets),
                           (uint32_t) n_packets, n_bytes, buf.as<unsigned long long>(), d_w);
    } else {
        const AedatSource src{d_payload, n_bytes, n_rec, nullptr, nullptr, 0u, nullptr};
        hipLaunchKernelGGL(aedat20_count_kernel, dim3((uint32_t) ((n_rec + AE_BLOCK - 1) / AE_BLOCK)), dim3(AE_T), 0, st, src, (uint32_t *) nullptr, d_w);
    }
    ECAL_HIP_TRY(ctx, hipGetLastError());
    AedatWords W;
    if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return rc;
    if (v31 && W.bad_table) {
        ctx->last_error = "aedat ingest: " + std::to_string(W.bad_table) + " packets of the table do not lie within the payload";
        return ECAL_ERR_INVALID;
    }
    *n_events = v31 ? W.n_slots : W.n_dvs;
    return ECAL_OK;
}

extern "C" int ecal_events_from_aedat_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_aedat_packet *d_packets,
                                          uint64_t n_packets, const ecal_aedat_options *opt, uint8_t *d_events, uint64_t capacity,
                                          ecal_aedat_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_aedat");
    if (!ctx) return ECAL_ERR_INVALID;
    ecal_aedat_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    int rc = aedat_check_args(ctx, d_payload, n_bytes, d_packets, n_packets, opt ? opt->format : ECAL_AEDAT_AUTO);
    if (rc) return rc;
    if ((rc = aedat_check_options(ctx, *opt))) return rc;
    if (capacity && !d_events) {
        ctx->last_error = "aedat ingest: null record buffer";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int st = aedat_ingest_any(ctx, opt->format, d_payload, n_bytes, reinterpret_cast<const AedatPacket *>(d_packets), n_packets, AE_NONE,
                                    *opt, d_events, capacity, nullptr, I, (hipStream_t) stream);
    if (info) *info = I;
    return st;
}

extern "C" int ecal_stream_create_from_aedat_file(ecal_ctx *ctx, const char *path, const ecal_aedat_options *opt, ecal_stream **out,
                                                  ecal_aedat_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_aedat_info I;
    memset(&I, 0, sizeof(I));
    const int rc = aedat_file_to_events(ctx, path, opt, &d_events, I);
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_aedat_file", d_events, I.n_events, out);
}

extern "C" int ecal_aedat_to_bin_file(ecal_ctx *ctx, const char *aedat_path, const char *bin_path, const ecal_aedat_options *opt,
                                      ecal_aedat_info *info) {
    if (!ctx || !aedat_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_aedat_info I;
    memset(&I, 0, sizeof(I));
    const int rc = aedat_file_to_events(ctx, aedat_path, opt, &d_events, I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_aedat_to_bin_file", d_events, I.n_events, bin_path);
}
