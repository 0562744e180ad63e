// Bag ingest (include/ecal.h, "bag ingest"): a ROS 1 bag (format 2.0) of dvs_msgs/EventArray messages resident in HBM into packed
// 25-byte records.  The field extraction, the filter, the field-list parser and the record walker are bag_events.hpp's (shared with
// the host decoder and the CPU test); design/16_bag_ingest.md has the reasoning.
//
// The record chain is NOT walked here: a message is found only through the record header before it, inside a chunk found the same
// way.  The host indexes the chosen messages (ecal_bag_index_messages) and the table comes in with the file.
//
// A block is BG_T threads x 4 consecutive slots = 1024 slots (ecal_bag_block_events).  A slot is an event of the table's slot space.
// Launches, with NO waiting between workgroups — state crosses blocks only between launches, or inside the one-workgroup scan:
//   1. bag_message_scan_kernel  one workgroup: the exclusive 64-bit scan of the table's n_events = every message's first slot; the
//                               table checked against n_bytes
//   2. bag_verdict_kernel       every slot classed; the kept events per block; the first slot that reaches end_time (64-bit atomic
//                               minimum)
//   3. ecal_scan_blocks         the blocks' first kept index
//   4. bag_write_kernel         classed again; the kept events below the first offender get their index (in-workgroup scan), are
//                               packed into LDS and copied out with aligned 32-bit stores; the totals
// "The stream ends here" is the test `slot < first offender` in pass 4, as in the raw and AEDAT ingests.  The host sees the counters
// once, behind pass 4 (ecal_events_from_bag_dev once more behind pass 1: the grid is a count of the table).
// The bodies of passes 2 and 4 are slot_kernels.hpp's (BagFormat below is this format's policy), the table scan, the table check, the
// bisection, the clipped load and the tails of passes 2 and 4 ingest_blocks.hpp's, the host driver ingest_driver.hpp's
// (ecal_ingest_message_table), all shared with the other table ingests; the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "slot_kernels.hpp"
#include "ingest_driver.hpp"
#include "bag_events.hpp"

namespace ecal {

using namespace ecal_bag;

static_assert(ECAL_ERR_INVALID == BAG_INVALID && ECAL_ERR_RANGE == BAG_RANGE && ECAL_OK == BAG_OK, "status codes");
static_assert(sizeof(ecal_bag_message) == 16 && sizeof(BagMessage) == 16, "message table entry");

constexpr int BG_T = BAG_BLOCK_THREADS;
constexpr uint32_t BG_PER = BAG_THREAD_EVENTS;
constexpr uint32_t BG_BLOCK = BAG_BLOCK_EVENTS;   // slots per block, and records staged in LDS (25 600 bytes: six workgroups a CU)
constexpr unsigned long long BG_NONE = ~0ull;

typedef MessageWords BagWords;   // the counters of one ingest (device)

// what a block kernel is given of the file
struct BagSource {
    const uint8_t *file;
    uint64_t n_bytes;
    uint64_t n_slots;                       // slots in all
    const BagMessage *messages;
    const unsigned long long *first;        // [n_messages + 1]
    uint32_t n_messages;
};

// The thread's slots: the four aligned words that hold each 13-byte record, shifted into x|y, secs, nsecs and the polarity byte.
struct BgSlots {
    uint32_t xy[BG_PER], secs[BG_PER], nsecs[BG_PER], pol[BG_PER];
    uint32_t n;      // slots of this thread in front of n_slots

    __device__ __forceinline__ BgSlots(const BagSource &src) {
        const uint64_t s0 = ((uint64_t) blockIdx.x * BG_T + threadIdx.x) * BG_PER;
        n = s0 < src.n_slots ? (uint32_t) (src.n_slots - s0 < BG_PER ? src.n_slots - s0 : BG_PER) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < BG_PER; j++) xy[j] = secs[j] = nsecs[j] = pol[j] = 0u;
        if (n) {
            // the block's messages by bisection (the same for every thread), the thread's inside them
            const uint64_t b0 = (uint64_t) blockIdx.x * BG_BLOCK;
            const uint64_t b1 = b0 + BG_BLOCK < src.n_slots ? b0 + BG_BLOCK - 1u : src.n_slots - 1u;
            const uint32_t m_lo = table_find(src.first, 0u, src.n_messages - 1u, b0);
            const uint32_t m_hi = table_find(src.first, m_lo, src.n_messages - 1u, b1);
            uint32_t m = table_find(src.first, m_lo, m_hi, s0);
            uint64_t m_first = src.first[m], m_next = src.first[m + 1], m_off = src.messages[m].offset;
#pragma unroll
            for (uint32_t j = 0; j < BG_PER; j++) {
                if (j < n) {
                    const uint64_t s = s0 + j;
                    if (s >= m_next) {   // (messages of no events in between are stepped over by the search)
                        m = table_find(src.first, m + 1u, m_hi, s);
                        m_first = src.first[m];
                        m_next = src.first[m + 1];
                        m_off = src.messages[m].offset;
                    }
                    // the record from aligned words, whatever its byte offset: r + 13 <= 16, so four words always suffice, and the
                    // first three lie wholly in front of the record's end.  A table that points behind the file (bad_table, an
                    // error on the host) reads zeros
                    const uint64_t off = m_off + (s - m_first) * BAG_EVENT_BYTES;
                    if (off + BAG_EVENT_BYTES <= src.n_bytes && off + BAG_EVENT_BYTES > off) {
                        const uint64_t al = off & ~3ull;
                        const uint32_t w0 = *reinterpret_cast<const uint32_t *>(src.file + al);
                        const uint32_t w1 = *reinterpret_cast<const uint32_t *>(src.file + al + 4u);
                        const uint32_t w2 = *reinterpret_cast<const uint32_t *>(src.file + al + 8u);
                        const uint32_t w3 = load32_clipped(src.file, al + 12u, src.n_bytes);
                        const uint32_t sh = 8u * (uint32_t) (off & 3u);
                        xy[j] = (uint32_t) ((((uint64_t) w1 << 32) | w0) >> sh);
                        secs[j] = (uint32_t) ((((uint64_t) w2 << 32) | w1) >> sh);
                        nsecs[j] = (uint32_t) ((((uint64_t) w3 << 32) | w2) >> sh);
                        pol[j] = (w3 >> sh) & 0xFFu;
                    }
                }
            }
        }
    }
    __device__ __forceinline__ BagEvent event(uint32_t j) const { return bag_event(xy[j], secs[j], nsecs[j], pol[j]); }
};

// the format of slot_kernels.hpp's bodies
struct BagFormat {
    typedef BagSource Source;
    typedef BagFilter Filter;
    typedef BagWords Words;
    typedef BgSlots Slots;
    static constexpr int T = BG_T, N_DROPS = 3;
    static constexpr uint32_t PER = BG_PER, BLOCK = BG_BLOCK;
    static constexpr uint8_t KEEP = BAG_CLASS_KEEP, STOP = BAG_CLASS_STOP;
    static __device__ __forceinline__ Slots slots(const Source &src, unsigned long long *) { return Slots(src); }
    static __device__ __forceinline__ bool is_event(const Slots &, uint32_t) { return true; }
    static __device__ __forceinline__ uint8_t classify(const Slots &s, uint32_t j, const Filter &flt, double *t, uint32_t *x, uint32_t *y) {
        return bag_classify(s.event(j), flt, t, x, y);
    }
    static __device__ __forceinline__ uint8_t polarity(const Slots &s, uint32_t j) { return (uint8_t) (s.pol[j] != 0u ? 1u : 0u); }
    static __device__ __forceinline__ constexpr uint8_t drop_class(int i) { return i == 0 ? BAG_CLASS_OUTSIDE : i == 1 ? BAG_CLASS_NEGATIVE : BAG_CLASS_BEFORE_START; }
    static __device__ __forceinline__ unsigned long long *drop_counter(Words *w, int i) { return i == 0 ? &w->n_outside : i == 1 ? &w->n_negative : &w->n_before_start; }
};

// first[m] = n_events of the messages before m, first[n] = all of them (table_exscan_1024); the table checked against n_bytes.
// One workgroup.
__global__ __launch_bounds__(1024) void bag_message_scan_kernel(const BagMessage *__restrict__ messages, uint32_t n, uint64_t n_bytes,
                                                                unsigned long long *__restrict__ first, BagWords *__restrict__ w) {
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (unsigned long long) messages[p].n_events; }, first);
    if (threadIdx.x == 0) w->n_slots = tot;
    // (a pass of its own, strided: the table is read once more than the scan needs; the scan's value_of runs twice an entry)
    const unsigned long long bad = table_count_outside(n, n_bytes, threadIdx.x, 1024u, [&](uint64_t p) { return messages[p].offset; },
                                                       [&](uint64_t p) { return (uint64_t) messages[p].n_events * BAG_EVENT_BYTES; });
    if (bad) atomicAdd(&w->bad_table, bad);
}

// the class of every slot, the kept events per block, the first slot that reaches end_time
__global__ __launch_bounds__(BG_T) void bag_verdict_kernel(BagSource src, BagFilter flt, uint32_t *__restrict__ blk_keep, BagWords *__restrict__ w) {
    slot_verdict_body<BagFormat>(src, flt, blk_keep, w);
}

// the kept events below the first offender, packed in LDS and copied out; the totals
__global__ __launch_bounds__(BG_T) void bag_write_kernel(BagSource src, const uint32_t *__restrict__ blk_koff, BagFilter flt,
                                                         uint8_t *__restrict__ events, uint64_t capacity, BagWords *__restrict__ w) {
    slot_write_body<BagFormat>(src, blk_koff, flt, events, capacity, w);
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_bag_default_options(ecal_bag_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->auto_time_base = 1;
    opt->start_time = -INFINITY;
}

extern "C" uint32_t ecal_bag_block_events(void) { return BG_BLOCK; }

namespace {

BagChoice bag_choice(const ecal_bag_options *o) {
    BagChoice ch;
    if (o && o->topic) ch.topic = o->topic;
    if (o && o->type) ch.type = o->type;
    return ch;
}

void bag_info_from_counts(ecal_bag_info &I, const BagCounts &c) {
    I.n_raw_events = c.n_raw_events;
    I.n_messages = c.n_messages;
    I.n_other_messages = c.n_other_messages;
    I.n_chunks = c.n_chunks;
    I.n_connections = c.n_connections;
    I.n_trailing_bytes = c.n_trailing_bytes;
    I.first_stamp_ns = c.first_stamp_ns;
    I.msg_width = c.msg_width;
    I.msg_height = c.msg_height;
}

int bag_check_args(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const void *d_messages, uint64_t n_messages) {
    const int rc = ecal_ingest_check_buffer(ctx, "bag ingest", d_file, n_bytes, 16, "file", "file's bytes");
    return rc ? rc : ecal_ingest_check_buffer(ctx, "bag ingest", d_messages, n_messages, 8, "message table", nullptr, "messages");
}

int bag_check_options(ecal_ctx *ctx, const ecal_bag_options &o) {
    if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) {
        ctx->last_error = "bag ingest: flip_x / flip_y need width / height";
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

const ecal_ingest_nouns BAG_NOUNS{"bag ingest", "bag", "message", "file", "message scan"};

void bag_launch_scan(const BagMessage *d_messages, uint64_t n_messages, uint64_t n_bytes, unsigned long long *first, BagWords *d_w, hipStream_t st) {
    hipLaunchKernelGGL(bag_message_scan_kernel, dim3(1), dim3(1024), 0, st, d_messages, (uint32_t) n_messages, n_bytes, first, d_w);
}

// o.time_base: the base in force (the caller has resolved auto_time_base).  n_slots_host, own_events: ecal_ingest_message_table's
int bag_ingest(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const BagMessage *d_messages, uint64_t n_messages, uint64_t n_slots_host,
               const ecal_bag_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events, ecal_bag_info &I, hipStream_t st) {
    I.n_messages = n_messages;
    I.time_base = o.time_base;
    const BagFilter flt{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
    return ecal_ingest_message_table<BagWords>(
        ctx, BAG_NOUNS, BagSource{d_file, n_bytes, 0, d_messages, nullptr, (uint32_t) n_messages}, flt, n_bytes, n_messages, BAG_EVENT_BYTES, n_slots_host,
        BG_BLOCK, d_events, capacity, own_events, I, st,
        [&](unsigned long long *first, BagWords *d_w) { bag_launch_scan(d_messages, n_messages, n_bytes, first, d_w, st); },
        [&](const BagSource &src, const BagFilter &f, uint32_t nb, uint32_t *keep, BagWords *d_w) {
            hipLaunchKernelGGL(bag_verdict_kernel, dim3(nb), dim3(BG_T), 0, st, src, f, keep, d_w);
        },
        [&](const BagSource &src, const BagFilter &f, uint32_t nb, const uint32_t *koff, uint8_t *events, uint64_t cap, BagWords *d_w) {
            hipLaunchKernelGGL(bag_write_kernel, dim3(nb), dim3(BG_T), 0, st, src, koff, f, events, cap, d_w);
        },
        [](const BagWords &, uint64_t *) { return ECAL_OK; });
}

// file -> (message table on the host, from record headers, beside the upload) -> file in HBM -> records in a device buffer of their
// own (null for none), the file's bytes freed
int bag_file_to_events(ecal_ctx *ctx, const char *path, const ecal_bag_options *opt, uint8_t **d_events, ecal_bag_info &I) {
    *d_events = nullptr;
    ecal_bag_options o;
    if (opt) o = *opt; else ecal_bag_default_options(&o);
    int rc = bag_check_options(ctx, o);
    if (rc) return rc;
    const BagChoice choice = bag_choice(&o);
    int fd;
    uint64_t file_bytes;
    {   // the first line in front of everything: a file of another kind is not uploaded
        std::vector<uint8_t> head;
        if ((rc = ecal_ingest_open_head(ctx, "bag ingest", path, 32, "cannot be read", &fd, &file_bytes, &head))) return rc;
        std::string err;
        if (bag_check_magic(head.data(), head.size(), &err)) {
            close(fd);
            ctx->last_error = "bag ingest: " + err + " (" + path + ")";
            return ECAL_ERR_INVALID;
        }
    }
    std::vector<BagMessage> table;
    BagCounts c;
    memset(&c, 0, sizeof(c));
    ecal_ingest_upload up;
    rc = ecal_ingest_upload_indexed(ctx, "bag", "bag ingest", "host message index", path, fd, 0, file_bytes, [&](std::string *error, const void **tab, size_t *tab_bytes) {
        ecal_ingest_file_reader rd{fd, file_bytes};
        std::string err;
        const int index_rc = bag_walk(rd, file_bytes, choice, c, [&](const BagMessage &m) { table.push_back(m); }, &err);
        if (index_rc) *error = "bag ingest: " + err + " (" + path + ")";
        *tab = table.data();
        *tab_bytes = table.size() * sizeof(BagMessage);
        return index_rc;
    }, &up);
    if (rc) return rc;
    bag_info_from_counts(I, c);
    o.time_base = bag_time_base(o.auto_time_base, o.time_base, c);
    I.time_base = o.time_base;
    const ecal_bag_info walked = I;
    rc = bag_ingest(ctx, up.d_file, up.n_bytes, (const BagMessage *) up.d_table, table.size(), c.n_raw_events, o, nullptr, 0, d_events, I, ctx->stream);
    I.n_messages = walked.n_messages;
    I.n_raw_events = walked.n_raw_events;
    ecal_ingest_free_upload(ctx, &up);
    return rc;
}

}  // namespace

extern "C" int ecal_bag_index_messages(ecal_ctx *ctx, const uint8_t *file_host, uint64_t n_bytes, const ecal_bag_options *opt, ecal_bag_message *out,
                                       uint64_t capacity, uint64_t *n_messages, ecal_bag_info *info) {
    if (!n_messages || (n_bytes && !file_host) || (capacity && !out)) return ECAL_ERR_INVALID;
    BagCounts c;
    memset(&c, 0, sizeof(c));
    std::string err;
    const int rc = bag_index_messages(file_host, n_bytes, bag_choice(opt), reinterpret_cast<BagMessage *>(out), capacity, n_messages, c, &err);
    if (rc && ctx) ctx->last_error = "ecal_bag_index_messages: " + err;
    if (info && rc != ECAL_ERR_INVALID) {
        memset(info, 0, sizeof(*info));
        bag_info_from_counts(*info, c);
    }
    return rc;
}

extern "C" int ecal_bag_count_events_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_bag_message *d_messages,
                                         uint64_t n_messages, uint64_t *n_events, void *stream) {
    if (!ctx || !n_events) return ECAL_ERR_INVALID;
    *n_events = 0;
    int rc = bag_check_args(ctx, d_file, n_bytes, d_messages, n_messages);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    if (!n_messages) return ECAL_OK;
    ecal_devbuf buf;
    BagWords W;
    if ((rc = ecal_ingest_scan_table(ctx, BAG_NOUNS, n_messages, buf, W, "", st, [&](unsigned long long *first, BagWords *d_w) {
            bag_launch_scan(reinterpret_cast<const BagMessage *>(d_messages), n_messages, n_bytes, first, d_w, st);
        })))
        return rc;
    *n_events = W.n_slots;
    return ECAL_OK;
}

extern "C" int ecal_events_from_bag_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_bag_message *d_messages,
                                        uint64_t n_messages, const ecal_bag_options *opt, uint8_t *d_events, uint64_t capacity,
                                        ecal_bag_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_bag");
    if (!ctx) return ECAL_ERR_INVALID;
    ecal_bag_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    if (!opt) {
        ctx->last_error = "bag ingest: no options (the device form needs an explicit time base)";
        return ECAL_ERR_INVALID;
    }
    int rc = bag_check_args(ctx, d_file, n_bytes, d_messages, n_messages);
    if (rc) return rc;
    if ((rc = bag_check_options(ctx, *opt))) return rc;
    if (opt->auto_time_base) {
        ctx->last_error = "bag ingest: the device form takes an explicit time base (auto_time_base must be 0; the indexer's first_stamp_ns is the automatic one)";
        return ECAL_ERR_INVALID;
    }
    if (capacity && !d_events) {
        ctx->last_error = "bag ingest: null record buffer";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int st = bag_ingest(ctx, d_file, n_bytes, reinterpret_cast<const BagMessage *>(d_messages), n_messages, BG_NONE, *opt, d_events, capacity,
                              nullptr, I, (hipStream_t) stream);
    if (info) *info = I;
    return st;
}

extern "C" int ecal_stream_create_from_bag_file(ecal_ctx *ctx, const char *path, const ecal_bag_options *opt, ecal_stream **out, ecal_bag_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_bag_info I;
    memset(&I, 0, sizeof(I));
    const int rc = bag_file_to_events(ctx, path, opt, &d_events, I);
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_bag_file", d_events, I.n_events, out);
}

extern "C" int ecal_bag_to_bin_file(ecal_ctx *ctx, const char *bag_path, const char *bin_path, const ecal_bag_options *opt, ecal_bag_info *info) {
    if (!ctx || !bag_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_bag_info I;
    memset(&I, 0, sizeof(I));
    const int rc = bag_file_to_events(ctx, bag_path, opt, &d_events, I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_bag_to_bin_file", d_events, I.n_events, bin_path);
}
