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
// The bodies of passes 3 and 5 are slot_kernels.hpp's (AedatFormat<FMT> below is this format's policy), the table scan, the table
// check, the bisection, the clipped load and the tails of passes 3 and 5 ingest_blocks.hpp's, the host drivers ingest_driver.hpp's (3.1:
// ecal_ingest_message_table, the bag ingest's whole path with packets for messages; 2.0: ecal_ingest_verdict_write behind its own
// front), all shared with the other table ingests; the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "slot_kernels.hpp"
#include "ingest_driver.hpp"
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

// the format of slot_kernels.hpp's bodies
template <int FMT> struct AedatFormat {
    typedef AedatSource Source;
    typedef AedatFilter Filter;
    typedef AedatWords Words;
    typedef AeSlots<FMT> Slots;
    static constexpr int T = AE_T, N_DROPS = 4;
    static constexpr uint32_t PER = AE_PER, BLOCK = AE_BLOCK;
    static constexpr uint8_t KEEP = AEDAT_CLASS_KEEP, STOP = AEDAT_CLASS_STOP;
    static __device__ __forceinline__ Slots slots(const Source &src, unsigned long long *s_scan) { return Slots(src, s_scan, true); }
    static __device__ __forceinline__ bool is_event(const Slots &s, uint32_t j) { return s.is_event(j); }
    static __device__ __forceinline__ uint8_t classify(const Slots &s, uint32_t j, const Filter &flt, double *t, uint32_t *x, uint32_t *y) {
        return aedat_classify(s.event(j), flt, t, x, y);
    }
    static __device__ __forceinline__ uint8_t polarity(const Slots &s, uint32_t j) {
        return (uint8_t) (FMT == AEDAT_FORMAT_31 ? (s.a[j] >> 1) & 1u : (s.a[j] >> 11) & 1u);
    }
    static __device__ __forceinline__ constexpr uint8_t drop_class(int i) {
        return i == 0 ? AEDAT_CLASS_INVALID : i == 1 ? AEDAT_CLASS_OUTSIDE : i == 2 ? AEDAT_CLASS_NEGATIVE : AEDAT_CLASS_BEFORE_START;
    }
    static __device__ __forceinline__ unsigned long long *drop_counter(Words *w, int i) {
        return i == 0 ? &w->n_invalid : i == 1 ? &w->n_outside : i == 2 ? &w->n_negative : &w->n_before_start;
    }
};

// first[p] = n_events of the packets before p, first[n] = all of them (table_exscan_1024); the table checked against n_bytes.
// One workgroup.
__global__ __launch_bounds__(1024) void aedat_packet_scan_kernel(const AedatPacket *__restrict__ packets, uint32_t n, uint64_t n_bytes,
                                                                 unsigned long long *__restrict__ first, AedatWords *__restrict__ w) {
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (unsigned long long) packets[p].n_events; }, first);
    if (threadIdx.x == 0) w->n_slots = tot;
    // (a pass of its own, strided: the table is read once more than the scan needs; the scan's value_of runs twice an entry)
    const unsigned long long bad = table_count_outside(n, n_bytes, threadIdx.x, 1024u, [&](uint64_t p) { return packets[p].offset; },
                                                       [&](uint64_t p) { return (uint64_t) packets[p].n_events * 8u; });
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
    slot_verdict_body<AedatFormat<FMT>>(src, flt, blk_keep, w);
}

// the kept events below the first offender, packed in LDS and copied out; the totals
template <int FMT>
__global__ __launch_bounds__(AE_T) void aedat_write_kernel(AedatSource src, const uint32_t *__restrict__ blk_koff, AedatFilter flt,
                                                           uint8_t *__restrict__ events, uint64_t capacity, AedatWords *__restrict__ w) {
    slot_write_body<AedatFormat<FMT>>(src, blk_koff, flt, events, capacity, w);
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

const ecal_ingest_nouns AEDAT_NOUNS{"aedat ingest", "aedat", "packet", "payload", "packet scan"};

AedatFilter aedat_filter(const ecal_aedat_options &o) {
    return AedatFilter{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
}

// 3.1: the message-table path, packets for messages.  n_slots_host, own_events: ecal_ingest_message_table's
int aedat31_ingest(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const AedatPacket *d_packets, uint64_t n_packets,
                   uint64_t n_slots_host, const ecal_aedat_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events,
                   ecal_aedat_info &I, hipStream_t st) {
    I.format = AEDAT_FORMAT_31;
    I.n_packets = n_packets;
    return ecal_ingest_message_table<AedatWords>(
        ctx, AEDAT_NOUNS, AedatSource{d_payload, n_bytes, 0, d_packets, nullptr, (uint32_t) n_packets, nullptr}, aedat_filter(o), n_bytes, n_packets, 8u,
        n_slots_host, AE_BLOCK, d_events, capacity, own_events, I, st,
        [&](unsigned long long *first, AedatWords *d_w) {
            hipLaunchKernelGGL(aedat_packet_scan_kernel, dim3(1), dim3(1024), 0, st, d_packets, (uint32_t) n_packets, n_bytes, first, d_w);
        },
        [&](const AedatSource &src, const AedatFilter &f, uint32_t nb, uint32_t *keep, AedatWords *d_w) {
            hipLaunchKernelGGL(aedat_verdict_kernel<AEDAT_FORMAT_31>, dim3(nb), dim3(AE_T), 0, st, src, f, keep, d_w);
        },
        [&](const AedatSource &src, const AedatFilter &f, uint32_t nb, const uint32_t *koff, uint8_t *events, uint64_t cap, AedatWords *d_w) {
            hipLaunchKernelGGL(aedat_write_kernel<AEDAT_FORMAT_31>, dim3(nb), dim3(AE_T), 0, st, src, koff, f, events, cap, d_w);
        },
        [&](const AedatWords &W, uint64_t *n_more) {
            I.n_invalid = *n_more = W.n_invalid;
            return ECAL_OK;
        });
}

// 2.0: the wrap count and its scan in front of the shared back half.  own_events != null: the records go into a buffer allocated here
// for the count (the caller's to hipFree, null when there is nothing to free); else into d_events / capacity
int aedat20_ingest(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_aedat_options &o, uint8_t *d_events, uint64_t capacity,
                   uint8_t **own_events, ecal_aedat_info &I, hipStream_t st) {
    I.format = AEDAT_FORMAT_20;
    if (own_events) *own_events = nullptr;
    I.n_records = n_bytes / 8u;
    I.n_trailing_bytes = n_bytes % 8u;
    if (!I.n_records) return ECAL_OK;
    if (I.n_records > 0xFFFFFFFFull) {
        I.n_events = I.n_records;
        ctx->last_error = "aedat ingest: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    const uint32_t nb = (uint32_t) ((I.n_records + AE_BLOCK - 1) / AE_BLOCK);
    ecal_load_timer tm("aedat", ctx->sw.load_trace, st);
    const size_t o_wr = 0, o_win = o_wr + up16((size_t) nb * 4), o_keep = o_win + up16(((size_t) nb + 1) * 4), o_koff = o_keep + up16((size_t) nb * 4),
                 o_words = o_koff + up16(((size_t) nb + 1) * 4), total = o_words + sizeof(AedatWords);
    ecal_devbuf scratch;
    int rc;
    if ((rc = ecal_ensure(ctx, scratch, total))) return rc;
    uint8_t *base = scratch.as<uint8_t>();
    uint32_t *wr = (uint32_t *) (base + o_wr), *win = (uint32_t *) (base + o_win), *keep = (uint32_t *) (base + o_keep),
             *koff = (uint32_t *) (base + o_koff);
    AedatWords *d_w = (AedatWords *) (base + o_words);
    const AedatFilter flt = aedat_filter(o);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(AedatWords), &d_w->first_stop, st))) return rc;
    tm.mark("start");
    const AedatSource src{d_payload, n_bytes, I.n_records, nullptr, nullptr, 0u, win};
    hipLaunchKernelGGL(aedat20_count_kernel, dim3(nb), dim3(AE_T), 0, st, src, wr, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark("wrap count");
    if ((rc = ecal_scan_blocks(ctx, wr, nb, win, st))) return rc;
    tm.mark("wrap scan");
    if (own_events) {   // the one count a size needs
        AedatWords W;
        if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return rc;
        capacity = W.n_dvs;
        if ((rc = ecal_ingest_alloc_records(ctx, "aedat ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    return ecal_ingest_verdict_write(
        ctx, "aedat ingest", tm, nb, keep, koff, (const AedatWords *) d_w, capacity, own_events, I, st,
        [&] { hipLaunchKernelGGL(aedat_verdict_kernel<AEDAT_FORMAT_20>, dim3(nb), dim3(AE_T), 0, st, src, flt, keep, d_w); },
        [&] { hipLaunchKernelGGL(aedat_write_kernel<AEDAT_FORMAT_20>, dim3(nb), dim3(AE_T), 0, st, src, (const uint32_t *) koff, flt, d_events, capacity, d_w); },
        [&](const AedatWords &W, uint64_t *n_more) -> int {
            I.n_other_records = W.n_other;
            I.n_raw_events = W.n_dvs;
            uint32_t wraps = 0;   // (the scan's total stands behind the blocks' offsets)
            ECAL_HIP_TRY(ctx, hipMemcpyAsync(&wraps, win + nb, 4, hipMemcpyDeviceToHost, st));
            ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
            I.n_time_wraps = wraps;
            I.n_invalid = *n_more = W.n_invalid;
            return ECAL_OK;
        });
}

int aedat_ingest_any(ecal_ctx *ctx, int format, const uint8_t *d_payload, uint64_t n_bytes, const AedatPacket *d_packets, uint64_t n_packets,
                     uint64_t n_slots_host, const ecal_aedat_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events,
                     ecal_aedat_info &I, hipStream_t st) {
    return format == ECAL_AEDAT_3_1 ? aedat31_ingest(ctx, d_payload, n_bytes, d_packets, n_packets, n_slots_host, o, d_events, capacity, own_events, I, st)
                                    : aedat20_ingest(ctx, d_payload, n_bytes, o, d_events, capacity, own_events, I, st);
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
        [&](uint64_t pos, uint8_t *raw) { return ecal_ingest_pread_all(fd, raw, AEDAT31_HEADER_BYTES, header_bytes + pos); }, file_bytes - header_bytes,
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
    int fd;
    uint64_t file_bytes;
    std::vector<uint8_t> head;
    if ((rc = ecal_ingest_open_head(ctx, "aedat ingest", path, 1u << 20, nullptr, &fd, &file_bytes, &head))) return rc;
    int format = ECAL_AEDAT_AUTO;
    uint64_t header_bytes = 0;
    std::string err;
    if (aedat_parse_header(head.data(), head.size(), head.size() == file_bytes, o.format, &format, &header_bytes, &err)) {
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
            const int index_rc = aedat_index_file(fd, header_bytes, file_bytes, o.source, table, c, path, error);
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
