// Mcap ingest (include/ecal_mcap.h): a ROS 2 MCAP recording of event messages resident in HBM into packed 25-byte records.  The
// container's walk, the schema parser, the CDR walk, the field extraction and the layouts are mcap_events.hpp's (shared with the host
// decoder and the CPU test); the filter is the bag ingest's (bag_events.hpp); design/25_mcap_ingest.md has the reasoning.
//
// The record chain is NOT walked here: the host indexes the chosen messages (ecal_mcap_index_messages) and the table comes in with
// the file.  STRUCT and MONO follow the bag ingest's device path.  A block is MC_T threads x 4 consecutive slots = 1024 slots
// (ecal_mcap_block_events); a slot is an event of the table's slot space.  Launches, with NO waiting between workgroups:
//   1. mcap_message_scan_kernel  one workgroup: the exclusive 64-bit scan of the table's n = every message's first slot; the table
//                                checked against n_bytes
//   2. mcap_verdict_kernel       every slot classed; the kept events per block; the first slot that reaches end_time
//   3. ecal_scan_blocks          the blocks' first kept index
//   4. mcap_write_kernel         classed again; the kept events below the first offender get their index, are packed into LDS and
//                                copied out with aligned stores; the totals
// The bodies of passes 2 and 4 are slot_kernels.hpp's (McapFormat<KIND> below is this format's policy), the table scan, the table check,
// the bisection, the clipped load and the tails ingest_blocks.hpp's, the host driver and the table scan's host side ingest_driver.hpp's
// (ecal_ingest_message_table, ecal_ingest_scan_table), all shared with the other table ingests.
// An event is fetched from the aligned load32_clipped words that cover it and its fields are shifted out of them (mcap_fetch_event):
// event 0 of a message and the later ones have their own offsets, and nothing in the file is aligned.
// EVT3: the same scan over the table's byte counts, then mcap_gather_kernel copies the messages' byte arrays, in file order, into one
// contiguous payload (any source alignment, one 16-byte store a thread), which ecal_events_from_raw_dev decodes: the decoder's state
// runs across message boundaries.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "../../include/ecal_mcap.h"
#include "slot_kernels.hpp"
#include "ingest_driver.hpp"
#include "mcap_events.hpp"

namespace ecal {

using namespace ecal_mcap;
using ecal_bag::bag_classify;
using ecal_bag::BAG_CLASS_KEEP;
using ecal_bag::BAG_CLASS_OUTSIDE;
using ecal_bag::BAG_CLASS_NEGATIVE;
using ecal_bag::BAG_CLASS_BEFORE_START;
using ecal_bag::BAG_CLASS_STOP;

static_assert(ECAL_ERR_INVALID == MCAP_INVALID && ECAL_ERR_RANGE == MCAP_RANGE && ECAL_OK == MCAP_OK, "status codes");
static_assert(sizeof(ecal_mcap_message) == 24 && sizeof(ecal_mcap_layout) == 32 && sizeof(ecal_mcap_info) == 184 && sizeof(ecal_mcap_options) == 64,
              "structures of ecal_mcap.h");
static_assert(ECAL_MCAP_STRUCT == MCAP_STRUCT && ECAL_MCAP_MONO == MCAP_MONO && ECAL_MCAP_EVT3 == MCAP_EVT3 && ECAL_MCAP_NONE == MCAP_NONE, "kinds");

constexpr int MC_T = MCAP_BLOCK_THREADS;
constexpr uint32_t MC_PER = MCAP_THREAD_EVENTS;
constexpr uint32_t MC_BLOCK = MCAP_BLOCK_EVENTS;   // slots per block, and records staged in LDS (25 600 bytes: six workgroups a CU)
constexpr unsigned long long MC_NONE = ~0ull;

typedef MessageWords McapWords;   // the counters of one ingest (device; EVT3: n_slots = payload bytes)

// what a block kernel is given of the file
struct McapSource {
    const uint8_t *file;
    uint64_t n_bytes;
    uint64_t n_slots;                       // slots in all (EVT3: payload bytes)
    const McapMessage *messages;
    const unsigned long long *first;        // [n_messages + 1]
    uint32_t n_messages;
    McapLayout layout;
};

// The thread's slots, each fetched through mcap_fetch_event.
template <uint32_t KIND> struct McSlots {
    BagEvent ev[MC_PER];
    uint32_t n;      // slots of this thread in front of n_slots

    __device__ __forceinline__ McSlots(const McapSource &src) {
        const uint64_t s0 = ((uint64_t) blockIdx.x * MC_T + threadIdx.x) * MC_PER;
        n = s0 < src.n_slots ? (uint32_t) (src.n_slots - s0 < MC_PER ? src.n_slots - s0 : MC_PER) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < MC_PER; j++) {
            ev[j].t_ns = 0;
            ev[j].x = ev[j].y = 0u;
            ev[j].pol = 0;
        }
        if (n) {
            // the block's messages by bisection (the same for every thread), the thread's inside them
            const uint64_t b0 = (uint64_t) blockIdx.x * MC_BLOCK;
            const uint64_t b1 = b0 + MC_BLOCK < src.n_slots ? b0 + MC_BLOCK - 1u : src.n_slots - 1u;
            const uint32_t m_lo = table_find(src.first, 0u, src.n_messages - 1u, b0);
            const uint32_t m_hi = table_find(src.first, m_lo, src.n_messages - 1u, b1);
            uint32_t m = table_find(src.first, m_lo, m_hi, s0);
            uint64_t m_first = src.first[m], m_next = src.first[m + 1], m_off = src.messages[m].offset;
            int64_t m_base = KIND == MCAP_MONO ? src.messages[m].time_base_ns : 0;
#pragma unroll
            for (uint32_t j = 0; j < MC_PER; j++) {
                if (j < n) {
                    const uint64_t s = s0 + j;
                    if (s >= m_next) {   // (messages of no events in between are stepped over by the search)
                        m = table_find(src.first, m + 1u, m_hi, s);
                        m_first = src.first[m];
                        m_next = src.first[m + 1];
                        m_off = src.messages[m].offset;
                        if (KIND == MCAP_MONO) m_base = src.messages[m].time_base_ns;
                    }
                    ev[j] = mcap_fetch_event<KIND>(src.file, src.n_bytes, src.layout, m_off, s - m_first, m_base);
                }
            }
        }
    }
    __device__ __forceinline__ const BagEvent &event(uint32_t j) const { return ev[j]; }
};

// the format of slot_kernels.hpp's bodies: the bag ingest's filter and classes
template <uint32_t KIND> struct McapFormat {
    typedef McapSource Source;
    typedef BagFilter Filter;
    typedef McapWords Words;
    typedef McSlots<KIND> Slots;
    static constexpr int T = MC_T, N_DROPS = 3;
    static constexpr uint32_t PER = MC_PER, BLOCK = MC_BLOCK;
    static constexpr uint8_t KEEP = BAG_CLASS_KEEP, STOP = BAG_CLASS_STOP;
    static __device__ __forceinline__ Slots slots(const Source &src, unsigned long long *) { return Slots(src); }
    static __device__ __forceinline__ bool is_event(const Slots &, uint32_t) { return true; }
    static __device__ __forceinline__ uint8_t classify(const Slots &s, uint32_t j, const Filter &flt, double *t, uint32_t *x, uint32_t *y) {
        return bag_classify(s.event(j), flt, t, x, y);
    }
    static __device__ __forceinline__ uint8_t polarity(const Slots &s, uint32_t j) { return s.event(j).pol; }
    static __device__ __forceinline__ constexpr uint8_t drop_class(int i) { return i == 0 ? BAG_CLASS_OUTSIDE : i == 1 ? BAG_CLASS_NEGATIVE : BAG_CLASS_BEFORE_START; }
    static __device__ __forceinline__ unsigned long long *drop_counter(Words *w, int i) { return i == 0 ? &w->n_outside : i == 1 ? &w->n_negative : &w->n_before_start; }
};

// first[m] = n of the messages before m, first[n] = all of them (table_exscan_1024); the table checked against n_bytes.  One workgroup.
__global__ __launch_bounds__(1024) void mcap_message_scan_kernel(const McapMessage *__restrict__ messages, uint32_t n, uint64_t n_bytes, McapLayout layout,
                                                                 unsigned long long *__restrict__ first, McapWords *__restrict__ w) {
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (unsigned long long) messages[p].n; }, first);
    if (threadIdx.x == 0) w->n_slots = tot;
    unsigned long long bad = table_count_outside(n, n_bytes, threadIdx.x, 1024u, [&](uint64_t p) { return messages[p].offset; },
                                                 [&](uint64_t p) { return mcap_message_bytes(layout, messages[p].n); });
    // EVT3: an odd byte count is a bad entry too (the gather moves whole 16-bit words).  A second walk over the table on purpose: the
    // shared check stays free of the format's own rule, and one workgroup over the table once more is nothing beside the gather
    if (layout.kind == MCAP_EVT3)
        for (uint64_t p = threadIdx.x; p < n; p += 1024u) bad += messages[p].n & 1u;
    if (bad) atomicAdd(&w->bad_table, bad);
}

// the class of every slot, the kept events per block, the first slot that reaches end_time
template <uint32_t KIND>
__global__ __launch_bounds__(MC_T) void mcap_verdict_kernel(McapSource src, BagFilter flt, uint32_t *__restrict__ blk_keep, McapWords *__restrict__ w) {
    slot_verdict_body<McapFormat<KIND>>(src, flt, blk_keep, w);
}

// the kept events below the first offender, packed in LDS and copied out; the totals
template <uint32_t KIND>
__global__ __launch_bounds__(MC_T) void mcap_write_kernel(McapSource src, const uint32_t *__restrict__ blk_koff, BagFilter flt, uint8_t *__restrict__ events,
                                                          uint64_t capacity, McapWords *__restrict__ w) {
    slot_write_body<McapFormat<KIND>>(src, blk_koff, flt, events, capacity, w);
}

// EVT3: bytes [16 q, 16 q + 16) of the payload, q = the thread's index in the grid, from the message(s) that hold them.  src.n_slots =
// the payload's bytes; every message's count is even, so a 16-bit word never straddles two messages.  dst: 16-byte aligned, room for
// the payload rounded up to 16; the bytes behind the payload's end are written as zeros.
__global__ __launch_bounds__(256) void mcap_gather_kernel(McapSource src, uint8_t *__restrict__ dst) {
    const uint64_t total = src.n_slots;
    const uint64_t d0 = ((uint64_t) blockIdx.x * 256u + threadIdx.x) * 16u;
    if (d0 >= total) return;
    const uint64_t d1 = d0 + 16u < total ? d0 + 16u : total;
    const uint64_t b0 = (uint64_t) blockIdx.x * MCAP_GATHER_BYTES;
    const uint64_t b1 = b0 + MCAP_GATHER_BYTES < total ? b0 + MCAP_GATHER_BYTES - 1u : total - 1u;
    const uint32_t m_lo = table_find(src.first, 0u, src.n_messages - 1u, b0);
    const uint32_t m_hi = table_find(src.first, m_lo, src.n_messages - 1u, b1);
    uint32_t m = table_find(src.first, m_lo, m_hi, d0);
    uint64_t m_first = src.first[m], m_next = src.first[m + 1], m_off = src.messages[m].offset;
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    if (d1 <= m_next) {   // one message holds them all: five aligned words shifted into four
        const uint64_t s = m_off + (d0 - m_first);
        const uint32_t nb = (uint32_t) (d1 - d0);
        if (s >= m_off && s + nb >= s && s + nb <= src.n_bytes) {
            const uint64_t al = s & ~3ull;
            const uint32_t sh = 8u * (uint32_t) (s & 3u);
            uint32_t wv[5];
#pragma unroll
            for (uint32_t i = 0; i < 5; i++) wv[i] = (i < 4 || sh) ? load32_clipped(src.file, al + 4u * i, src.n_bytes) : 0u;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t v = (uint32_t) ((((uint64_t) wv[i + 1] << 32) | wv[i]) >> sh);
                out[i] = 4u * i + 4u <= nb ? v : 4u * i < nb ? v & 0xFFFFu : 0u;   // (nb is even)
            }
        }
    } else {              // word by word through the messages
#pragma unroll
        for (uint32_t h = 0; h < 8; h++) {
            const uint64_t d = d0 + 2u * h;
            if (d < total) {
                if (d >= m_next) {
                    m = table_find(src.first, m + 1u, m_hi, d);
                    m_first = src.first[m];
                    m_next = src.first[m + 1];
                    m_off = src.messages[m].offset;
                }
                const uint64_t s = m_off + (d - m_first);
                const uint32_t v = (s >= m_off && s + 2u > s && s + 2u <= src.n_bytes) ? mcap_load_field(src.file, s, 2u, src.n_bytes) : 0u;
                out[h >> 1] |= v << (16u * (h & 1u));
            }
        }
    }
    *reinterpret_cast<uint4 *>(dst + d0) = make_uint4(out[0], out[1], out[2], out[3]);
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_mcap_default_options(ecal_mcap_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->auto_time_base = 1;
    opt->start_time = -INFINITY;
}

extern "C" uint32_t ecal_mcap_block_events(void) { return MC_BLOCK; }

namespace {

const char WHO[] = "mcap ingest";
const ecal_ingest_nouns MCAP_NOUNS{WHO, "mcap", "message", "file", "message scan"};

McapLayout mcap_layout_of(const ecal_mcap_layout &l) {
    McapLayout L;
    memcpy(&L, &l, sizeof(L));
    return L;
}

void mcap_info_from_counts(ecal_mcap_info &I, const McapCounts &c) {
    I.n_raw_events = c.n_raw_events;
    I.n_messages = c.n_messages;
    I.n_other_messages = c.n_other_messages;
    I.n_chunks = c.n_chunks;
    I.n_schemas = c.n_schemas;
    I.n_channels = c.n_channels;
    I.n_trailing_bytes = c.n_trailing_bytes;
    I.first_stamp_ns = c.first_stamp_ns;
    I.msg_width = c.msg_width;
    I.msg_height = c.msg_height;
    I.n_payload_bytes = c.n_payload_bytes;
    memcpy(&I.layout, &c.layout, sizeof(I.layout));
}

int mcap_check_args(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const void *d_messages, uint64_t n_messages, const ecal_mcap_layout *layout) {
    int rc = ecal_ingest_check_buffer(ctx, WHO, d_file, n_bytes, 16, "file", "file's bytes");
    if (!rc) rc = ecal_ingest_check_buffer(ctx, WHO, d_messages, n_messages, 8, "message table", nullptr, "messages");
    if (rc) return rc;
    if (!layout) {
        ctx->last_error = std::string(WHO) + ": null layout (the indexer's info.layout)";
        return ECAL_ERR_INVALID;
    }
    const char *why = nullptr;
    if (n_messages && !mcap_layout_valid(mcap_layout_of(*layout), &why)) {
        ctx->last_error = std::string(WHO) + ": the layout has " + why;
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

int mcap_check_options(ecal_ctx *ctx, const ecal_mcap_options &o) {
    if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) {
        ctx->last_error = std::string(WHO) + ": flip_x / flip_y need width / height";
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

// the scan of the table alone: W.n_slots and W.bad_table on the host (count_events_dev, and the front of the EVT3 path); `first` stays
// in `scratch` for the gather
int mcap_scan_table(ecal_ctx *ctx, const McapMessage *d_messages, uint64_t n_messages, uint64_t n_bytes, const McapLayout &L, ecal_devbuf &scratch,
                    McapWords &W, hipStream_t st) {
    return ecal_ingest_scan_table(ctx, MCAP_NOUNS, n_messages, scratch, W, L.kind == MCAP_EVT3 ? " or have an odd byte count" : "", st,
                                  [&](unsigned long long *first, McapWords *d_w) {
                                      hipLaunchKernelGGL(mcap_message_scan_kernel, dim3(1), dim3(1024), 0, st, d_messages, (uint32_t) n_messages, n_bytes, L, first, d_w);
                                  });
}

// EVT3: the table's byte arrays into one payload of its own (*payload, hipMalloc; null for no bytes), *total its bytes
int mcap_gather(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const McapMessage *d_messages, uint64_t n_messages, const McapLayout &L,
                uint8_t **payload, uint64_t *total, hipStream_t st) {
    *payload = nullptr;
    *total = 0;
    ecal_devbuf scratch;
    McapWords W;
    int rc = mcap_scan_table(ctx, d_messages, n_messages, n_bytes, L, scratch, W, st);
    if (rc) return rc;
    if (W.n_slots > n_bytes) {   // (messages that overlap)
        ctx->last_error = std::string(WHO) + ": the message table names more payload bytes than the file holds";
        return ECAL_ERR_INVALID;
    }
    if (!W.n_slots) return ECAL_OK;
    hipError_t e = hipMalloc((void **) payload, up16((size_t) W.n_slots) + 16);
    if (e != hipSuccess) {
        *payload = nullptr;
        ctx->last_error = std::string(WHO) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
    }
    ecal_load_timer tm("mcap", ctx->sw.load_trace, st);
    tm.mark("start");
    const McapSource src{d_file, n_bytes, W.n_slots, d_messages, scratch.as<unsigned long long>(), (uint32_t) n_messages, L};
    const uint64_t nb = (W.n_slots + MCAP_GATHER_BYTES - 1) / MCAP_GATHER_BYTES;
    hipLaunchKernelGGL(mcap_gather_kernel, dim3((uint32_t) nb), dim3(256), 0, st, src, *payload);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) {
        tm.mark("gather");
        le = hipStreamSynchronize(st);   // (`first` lives in `scratch`, which goes with this frame)
    }
    if (le != hipSuccess) {
        (void) hipFree(*payload);
        *payload = nullptr;
        ctx->last_error = std::string(WHO) + ": " + hipGetErrorString(le);
        return ECAL_ERR_HIP;
    }
    *total = W.n_slots;
    return ECAL_OK;
}

void mcap_info_from_raw(ecal_mcap_info &I, const ecal_raw_info &R, uint64_t total) {
    I.n_events = R.n_events;
    I.n_outside = R.n_outside;
    I.n_negative = R.n_negative;
    I.n_before_start = R.n_before_start;
    I.n_after_end = R.n_after_end;
    I.n_no_state = R.n_no_state;
    I.n_other_words = R.n_other_words;
    I.n_time_wraps = R.n_time_wraps;
    I.n_payload_bytes = total;
    I.n_raw_events = R.n_events + R.n_outside + R.n_negative + R.n_before_start + R.n_after_end + R.n_no_state;
}

// EVT3, both forms.  own_events != null: the records go into a buffer allocated here for the payload's count
int mcap_ingest_evt3(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const McapMessage *d_messages, uint64_t n_messages, const McapLayout &L,
                     const ecal_mcap_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events, ecal_mcap_info &I, hipStream_t st) {
    if (own_events) *own_events = nullptr;
    if (o.flip_x || o.flip_y) {
        ctx->last_error = std::string(WHO) + ": flip_x / flip_y are not available for evt3 packets";
        return ECAL_ERR_INVALID;
    }
    uint8_t *payload = nullptr;
    uint64_t total = 0;
    int rc = mcap_gather(ctx, d_file, n_bytes, d_messages, n_messages, L, &payload, &total, st);
    if (rc) return rc;
    I.n_payload_bytes = total;
    if (!total) return ECAL_OK;
    ecal_raw_options ro;
    ecal_raw_default_options(&ro);
    ro.format = ECAL_RAW_EVT3;
    ro.time_base = o.time_base;
    ro.width = o.width;
    ro.height = o.height;
    ro.start_time = o.start_time;
    ro.has_end_time = o.has_end_time;
    ro.end_time = o.end_time;
    if (own_events) {
        uint64_t n = 0;
        rc = ecal_raw_count_events_dev(ctx, payload, total, ECAL_RAW_EVT3, &n, st);
        if (!rc && n) rc = ecal_ingest_alloc_records(ctx, WHO, n, own_events);
        capacity = n;
        d_events = *own_events;
    }
    ecal_raw_info R;
    memset(&R, 0, sizeof(R));
    if (!rc) rc = ecal_events_from_raw_dev(ctx, payload, total, &ro, d_events, capacity, &R, st);
    (void) hipFree(payload);
    if (rc == ECAL_OK || rc == ECAL_ERR_RANGE) mcap_info_from_raw(I, R, total);
    return rc ? ecal_ingest_drop_records(own_events, rc) : rc;
}

// STRUCT and MONO: the bag ingest's device path.  o.time_base: the base in force.  n_slots_host, own_events: ecal_ingest_message_table's
template <uint32_t KIND>
int mcap_ingest(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const McapMessage *d_messages, uint64_t n_messages, uint64_t n_slots_host,
                const McapLayout &L, const ecal_mcap_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events, ecal_mcap_info &I,
                hipStream_t st) {
    const BagFilter flt{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
    return ecal_ingest_message_table<McapWords>(
        ctx, MCAP_NOUNS, McapSource{d_file, n_bytes, 0, d_messages, nullptr, (uint32_t) n_messages, L}, flt, n_bytes, n_messages,
        std::min(L.span[0], L.span[1]), n_slots_host, MC_BLOCK, d_events, capacity, own_events, I, st,
        [&](unsigned long long *first, McapWords *d_w) {
            hipLaunchKernelGGL(mcap_message_scan_kernel, dim3(1), dim3(1024), 0, st, d_messages, (uint32_t) n_messages, n_bytes, L, first, d_w);
        },
        [&](const McapSource &src, const BagFilter &f, uint32_t nb, uint32_t *keep, McapWords *d_w) {
            hipLaunchKernelGGL(mcap_verdict_kernel<KIND>, dim3(nb), dim3(MC_T), 0, st, src, f, keep, d_w);
        },
        [&](const McapSource &src, const BagFilter &f, uint32_t nb, const uint32_t *koff, uint8_t *events, uint64_t cap, McapWords *d_w) {
            hipLaunchKernelGGL(mcap_write_kernel<KIND>, dim3(nb), dim3(MC_T), 0, st, src, koff, f, events, cap, d_w);
        },
        [](const McapWords &, uint64_t *) { return ECAL_OK; });
}

// by kind; I.n_messages, I.time_base and I.layout are set here
int mcap_ingest_any(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const McapMessage *d_messages, uint64_t n_messages, uint64_t n_slots_host,
                    const McapLayout &L, const ecal_mcap_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events, ecal_mcap_info &I,
                    hipStream_t st) {
    if (own_events) *own_events = nullptr;
    I.n_messages = n_messages;
    I.time_base = o.time_base;
    memcpy(&I.layout, &L, sizeof(I.layout));
    if (!n_messages) return ECAL_OK;
    if (L.kind == MCAP_EVT3) return mcap_ingest_evt3(ctx, d_file, n_bytes, d_messages, n_messages, L, o, d_events, capacity, own_events, I, st);
    return L.kind == MCAP_MONO
               ? mcap_ingest<MCAP_MONO>(ctx, d_file, n_bytes, d_messages, n_messages, n_slots_host, L, o, d_events, capacity, own_events, I, st)
               : mcap_ingest<MCAP_STRUCT>(ctx, d_file, n_bytes, d_messages, n_messages, n_slots_host, L, o, d_events, capacity, own_events, I, st);
}

// file -> (message table on the host, beside the upload) -> file in HBM -> records in a device buffer of their own (null for none), the
// file's bytes freed
int mcap_file_to_events(ecal_ctx *ctx, const char *path, const ecal_mcap_options *opt, uint8_t **d_events, ecal_mcap_info &I) {
    *d_events = nullptr;
    ecal_mcap_options o;
    if (opt) o = *opt; else ecal_mcap_default_options(&o);
    int rc = mcap_check_options(ctx, o);
    if (rc) return rc;
    const std::string topic = o.topic ? o.topic : "";
    int fd;
    uint64_t file_bytes;
    {   // the magic in front of everything: a file of another kind is not uploaded
        std::vector<uint8_t> head;
        if ((rc = ecal_ingest_open_head(ctx, WHO, path, 16, "cannot be read", &fd, &file_bytes, &head))) return rc;
        std::string err;
        if (mcap_check_magic(head.data(), head.size(), &err)) {
            close(fd);
            ctx->last_error = std::string(WHO) + ": " + err + " (" + path + ")";
            return ECAL_ERR_INVALID;
        }
    }
    std::vector<McapMessage> table;
    McapCounts c;
    memset(&c, 0, sizeof(c));
    ecal_ingest_upload up;
    rc = ecal_ingest_upload_indexed(ctx, "mcap", WHO, "host message index", path, fd, 0, file_bytes, [&](std::string *error, const void **tab, size_t *tab_bytes) {
        ecal_ingest_file_reader rd{fd, file_bytes};
        std::string err;
        const int index_rc = mcap_walk(rd, file_bytes, topic, c, [&](const McapMessage &m) { table.push_back(m); }, &err);
        if (index_rc) *error = std::string(WHO) + ": " + err + " (" + path + ")";
        *tab = table.data();
        *tab_bytes = table.size() * sizeof(McapMessage);
        return index_rc;
    }, &up);
    if (rc) return rc;
    mcap_info_from_counts(I, c);
    o.time_base = mcap_time_base(o.auto_time_base, o.time_base, c);
    I.time_base = o.time_base;
    const ecal_mcap_info walked = I;
    rc = mcap_ingest_any(ctx, up.d_file, up.n_bytes, (const McapMessage *) up.d_table, table.size(), c.layout.kind == MCAP_EVT3 ? MC_NONE : c.n_raw_events, c.layout, o,
                         nullptr, 0, d_events, I, ctx->stream);
    I.n_messages = walked.n_messages;
    if (c.layout.kind != MCAP_EVT3) I.n_raw_events = walked.n_raw_events;
    ecal_ingest_free_upload(ctx, &up);
    return rc;
}

}  // namespace

extern "C" int ecal_mcap_index_messages(ecal_ctx *ctx, const uint8_t *file_host, uint64_t n_bytes, const ecal_mcap_options *opt, ecal_mcap_message *out,
                                        uint64_t capacity, uint64_t *n_messages, ecal_mcap_info *info) {
    if (!n_messages || (n_bytes && !file_host) || (capacity && !out)) return ECAL_ERR_INVALID;
    McapCounts c;
    memset(&c, 0, sizeof(c));
    std::string err;
    const int rc = mcap_index_messages(file_host, n_bytes, opt && opt->topic ? opt->topic : "", reinterpret_cast<McapMessage *>(out), capacity, n_messages, c, &err);
    if (rc && ctx) ctx->last_error = "ecal_mcap_index_messages: " + err;
    if (info && rc != ECAL_ERR_INVALID) {
        memset(info, 0, sizeof(*info));
        mcap_info_from_counts(*info, c);
    }
    return rc;
}

extern "C" int ecal_mcap_count_events_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_mcap_message *d_messages,
                                          uint64_t n_messages, const ecal_mcap_layout *layout, uint64_t *n_events, void *stream) {
    if (!ctx || !n_events) return ECAL_ERR_INVALID;
    *n_events = 0;
    int rc = mcap_check_args(ctx, d_file, n_bytes, d_messages, n_messages, layout);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    if (!n_messages) return ECAL_OK;
    const McapLayout L = mcap_layout_of(*layout);
    const McapMessage *msgs = reinterpret_cast<const McapMessage *>(d_messages);
    if (L.kind == MCAP_EVT3) {
        uint8_t *payload = nullptr;
        uint64_t total = 0;
        if ((rc = mcap_gather(ctx, d_file, n_bytes, msgs, n_messages, L, &payload, &total, st))) return rc;
        if (total) rc = ecal_raw_count_events_dev(ctx, payload, total, ECAL_RAW_EVT3, n_events, st);
        if (payload) (void) hipFree(payload);
        return rc;
    }
    ecal_devbuf buf;
    McapWords W;
    if ((rc = mcap_scan_table(ctx, msgs, n_messages, n_bytes, L, buf, W, st))) return rc;
    *n_events = W.n_slots;
    return ECAL_OK;
}

extern "C" int ecal_events_from_mcap_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_mcap_message *d_messages,
                                         uint64_t n_messages, const ecal_mcap_layout *layout, const ecal_mcap_options *opt, uint8_t *d_events,
                                         uint64_t capacity, ecal_mcap_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_mcap");
    if (!ctx) return ECAL_ERR_INVALID;
    ecal_mcap_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    if (!opt) {
        ctx->last_error = std::string(WHO) + ": no options (the device form needs an explicit time base)";
        return ECAL_ERR_INVALID;
    }
    int rc = mcap_check_args(ctx, d_file, n_bytes, d_messages, n_messages, layout);
    if (rc) return rc;
    if ((rc = mcap_check_options(ctx, *opt))) return rc;
    if (opt->auto_time_base) {
        ctx->last_error = std::string(WHO) + ": the device form takes an explicit time base (auto_time_base must be 0; the indexer's first_stamp_ns is the automatic one, 0 for evt3)";
        return ECAL_ERR_INVALID;
    }
    if (capacity && !d_events) {
        ctx->last_error = std::string(WHO) + ": null record buffer";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int st = mcap_ingest_any(ctx, d_file, n_bytes, reinterpret_cast<const McapMessage *>(d_messages), n_messages, MC_NONE, mcap_layout_of(*layout), *opt,
                                   d_events, capacity, nullptr, I, (hipStream_t) stream);
    if (info) *info = I;
    return st;
}

extern "C" int ecal_stream_create_from_mcap_file(ecal_ctx *ctx, const char *path, const ecal_mcap_options *opt, ecal_stream **out, ecal_mcap_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_mcap_info I;
    memset(&I, 0, sizeof(I));
    const int rc = mcap_file_to_events(ctx, path, opt, &d_events, I);
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_mcap_file", d_events, I.n_events, out);
}

extern "C" int ecal_mcap_to_bin_file(ecal_ctx *ctx, const char *mcap_path, const char *bin_path, const ecal_mcap_options *opt, ecal_mcap_info *info) {
    if (!ctx || !mcap_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_mcap_info I;
    memset(&I, 0, sizeof(I));
    const int rc = mcap_file_to_events(ctx, mcap_path, opt, &d_events, I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_mcap_to_bin_file", d_events, I.n_events, bin_path);
}
