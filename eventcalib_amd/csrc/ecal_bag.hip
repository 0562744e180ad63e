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
// The table scan, the bisection, the clipped load and the tails of passes 2 and 4 are ingest_blocks.hpp's, shared with the other
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
#include "bag_events.hpp"

namespace ecal {

using namespace ecal_bag;

static_assert(ECAL_ERR_INVALID == BAG_INVALID && ECAL_ERR_RANGE == BAG_RANGE && ECAL_OK == BAG_OK, "status codes");
static_assert(sizeof(ecal_bag_message) == 16 && sizeof(BagMessage) == 16, "message table entry");

constexpr int BG_T = BAG_BLOCK_THREADS;
constexpr uint32_t BG_PER = BAG_THREAD_EVENTS;
constexpr uint32_t BG_BLOCK = BAG_BLOCK_EVENTS;   // slots per block, and records staged in LDS (25 600 bytes: six workgroups a CU)
constexpr unsigned long long BG_NONE = ~0ull;

// the counters of one ingest (device)
struct BagWords {
    unsigned long long n_slots;      // slots of the table
    unsigned long long first_stop;   // the first slot that reaches end_time (BG_NONE: none)
    unsigned long long n_events, n_outside, n_negative, n_before_start;
    unsigned long long bad_table;    // messages of the table that do not lie within n_bytes
};

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

// first[m] = n_events of the messages before m, first[n] = all of them (table_exscan_1024); the table checked against n_bytes.
// One workgroup.
__global__ __launch_bounds__(1024) void bag_message_scan_kernel(const BagMessage *__restrict__ messages, uint32_t n, uint64_t n_bytes,
                                                                unsigned long long *__restrict__ first, BagWords *__restrict__ w) {
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (unsigned long long) messages[p].n_events; }, first);
    if (threadIdx.x == 0) w->n_slots = tot;
    // (a pass of its own, strided: the table is read once more than the scan needs; the scan's value_of runs twice an entry)
    unsigned long long bad = 0;
    for (uint64_t p = threadIdx.x; p < n; p += 1024u) {
        const uint64_t off = messages[p].offset, len = (uint64_t) messages[p].n_events * BAG_EVENT_BYTES;
        if (off > n_bytes || len > n_bytes - off) bad++;
    }
    if (bad) atomicAdd(&w->bad_table, bad);
}

// the class of every slot, the kept events per block, the first slot that reaches end_time
__global__ __launch_bounds__(BG_T) void bag_verdict_kernel(BagSource src, BagFilter flt, uint32_t *__restrict__ blk_keep, BagWords *__restrict__ w) {
    const int tid = threadIdx.x;
    const BgSlots mine(src);
    uint32_t keep = 0, stop = 0xFFFFFFFFu;   // (stop: a slot within the block)
#pragma unroll
    for (uint32_t j = 0; j < BG_PER; j++) {
        if (j < mine.n) {
            double t;
            uint32_t x, y;
            const uint8_t c = bag_classify(mine.event(j), flt, &t, &x, &y);
            keep += c == BAG_CLASS_KEEP ? 1u : 0u;
            const uint32_t at = (uint32_t) tid * BG_PER + j;
            if (c == BAG_CLASS_STOP && at < stop) stop = at;
        }
    }
    block_keep_and_stop<BG_T>(keep, stop, blk_keep, &w->first_stop, [] { return (unsigned long long) blockIdx.x * BG_BLOCK; });
}

// the kept events below the first offender, packed in LDS and copied out; the totals
__global__ __launch_bounds__(BG_T) void bag_write_kernel(BagSource src, const uint32_t *__restrict__ blk_koff, BagFilter flt,
                                                         uint8_t *__restrict__ events, uint64_t capacity, BagWords *__restrict__ w) {
    __shared__ unsigned long long s_scan[BG_T / 64];
    __shared__ uint32_t s_cnt[3];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[BG_BLOCK * 25];
    const int tid = threadIdx.x;
    const unsigned long long X = w->first_stop;
    const uint64_t slot0 = (uint64_t) blockIdx.x * BG_BLOCK;
    if (slot0 >= X) return;   // (the whole block lies behind the offender; the same for every thread)
    const BgSlots mine(src);
    // slots of this block below the offender: in-block slot < lim
    const uint32_t lim = X - slot0 < (unsigned long long) BG_BLOCK ? (uint32_t) (X - slot0) : BG_BLOCK;
    if (tid < 3) s_cnt[tid] = 0;
    uint32_t keep = 0, kept_mask = 0, drop[3] = {0u, 0u, 0u};
    double kt[BG_PER];
    uint32_t kx[BG_PER], ky[BG_PER];
#pragma unroll
    for (uint32_t j = 0; j < BG_PER; j++) {
        kt[j] = 0.0;
        kx[j] = ky[j] = 0u;
        if (j < mine.n && (uint32_t) tid * BG_PER + j < lim) {
            const uint8_t c = bag_classify(mine.event(j), flt, &kt[j], &kx[j], &ky[j]);
            if (c == BAG_CLASS_KEEP) {
                keep++;
                kept_mask |= 1u << j;
            }
            drop[0] += c == BAG_CLASS_OUTSIDE ? 1u : 0u;
            drop[1] += c == BAG_CLASS_NEGATIVE ? 1u : 0u;
            drop[2] += c == BAG_CLASS_BEFORE_START ? 1u : 0u;
        }
    }
    uint32_t kex, eb, ktot, tb;
    block_exscan_pair<BG_T>(keep, 0u, s_scan, &kex, &eb, &ktot, &tb);   // (its barriers order the zeroing of s_cnt too)
    block_add_drops<3>(drop, s_cnt);
    // at most BG_BLOCK kept events: one chunk of LDS holds them all
    uint32_t k = kex;
#pragma unroll
    for (uint32_t j = 0; j < BG_PER; j++) {
        if (kept_mask >> j & 1u) {
            pack_record(s_rec + k * 25u, kt[j], (double) kx[j], (double) ky[j], (uint8_t) (mine.pol[j] != 0u ? 1u : 0u));
            k++;
        }
    }
    __syncthreads();
    if (tid < 3 && s_cnt[tid])
        atomicAdd(tid == 0 ? &w->n_outside : tid == 1 ? &w->n_negative : &w->n_before_start, (unsigned long long) s_cnt[tid]);
    if (tid == 0 && ktot) atomicAdd(&w->n_events, (unsigned long long) ktot);
    block_copy_out<BG_T>(s_rec, ktot, events, blk_koff[blockIdx.x], capacity);
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

// o.time_base: the base in force (the caller has resolved auto_time_base).
// n_slots_host: the sum of the table's n_events when the caller knows it (the file forms), else BG_NONE.
// own_events != null: the records go into a buffer allocated here for the count (the caller's to hipFree, null when there is
// nothing to free); else into d_events / capacity
int bag_ingest(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const BagMessage *d_messages, uint64_t n_messages, uint64_t n_slots_host,
               const ecal_bag_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events, ecal_bag_info &I, hipStream_t st) {
    if (own_events) *own_events = nullptr;
    I.n_messages = n_messages;
    I.time_base = o.time_base;
    if (!n_messages || n_slots_host == 0) return ECAL_OK;
    // no fewer than the slots: sizes the per-block arrays
    const uint64_t bound = n_slots_host != BG_NONE ? n_slots_host : std::min<uint64_t>(n_bytes / BAG_EVENT_BYTES, 0xFFFFFFFFull);
    if (bound > 0xFFFFFFFFull) {
        I.n_events = bound;
        ctx->last_error = "bag ingest: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    const uint32_t nb_max = (uint32_t) ((bound + BG_BLOCK - 1) / BG_BLOCK);
    ecal_load_timer tm("bag", ctx->sw.load_trace, st);
    const size_t o_first = 0, o_keep = o_first + up16((size_t) (n_messages + 1) * 8), o_koff = o_keep + up16(((size_t) nb_max + 1) * 4),
                 o_words = o_koff + up16(((size_t) nb_max + 1) * 4), total = o_words + sizeof(BagWords);
    ecal_devbuf scratch;
    int rc;
    if ((rc = ecal_ensure(ctx, scratch, total))) return rc;
    uint8_t *base = scratch.as<uint8_t>();
    unsigned long long *first = (unsigned long long *) (base + o_first);
    uint32_t *keep = (uint32_t *) (base + o_keep), *koff = (uint32_t *) (base + o_koff);
    BagWords *d_w = (BagWords *) (base + o_words);
    const BagFilter flt{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(BagWords), &d_w->first_stop, st))) return rc;
    tm.mark("start");
    BagSource src{d_file, n_bytes, bound, d_messages, first, (uint32_t) n_messages};
    BagWords W;
    auto fetch = [&]() { return ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st); };
    uint32_t nb = nb_max;
    hipLaunchKernelGGL(bag_message_scan_kernel, dim3(1), dim3(1024), 0, st, d_messages, (uint32_t) n_messages, n_bytes, first, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark("message scan");
    if (n_slots_host == BG_NONE) {   // the grid is a count of the table: one look at it
        if ((rc = fetch())) return rc;
        if (W.bad_table) {
            ctx->last_error = "bag ingest: " + std::to_string(W.bad_table) + " messages of the table do not lie within the file";
            return ECAL_ERR_INVALID;
        }
        if (W.n_slots > 0xFFFFFFFFull) {
            I.n_events = W.n_slots;
            ctx->last_error = "bag ingest: more than 2^32-1 events";
            return ECAL_ERR_RANGE;
        }
        if (W.n_slots > bound) {   // (messages that overlap: more events than the file has room for)
            ctx->last_error = "bag ingest: the message table names more events than the file holds";
            return ECAL_ERR_INVALID;
        }
        src.n_slots = W.n_slots;
        nb = (uint32_t) ((W.n_slots + BG_BLOCK - 1) / BG_BLOCK);
    }
    I.n_raw_events = src.n_slots;
    if (!src.n_slots) return ECAL_OK;
    if (own_events) {
        capacity = src.n_slots;
        if ((rc = ecal_ingest_alloc_records(ctx, "bag ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    auto fail = [&](int code) { return ecal_ingest_drop_records(own_events, code); };
    auto launched = [&]() -> int {
        ECAL_HIP_TRY(ctx, hipGetLastError());
        return ECAL_OK;
    };
    hipLaunchKernelGGL(bag_verdict_kernel, dim3(nb), dim3(BG_T), 0, st, src, flt, keep, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("verdict");
    if ((rc = ecal_scan_blocks(ctx, keep, nb, koff, st))) return fail(rc);
    hipLaunchKernelGGL(bag_write_kernel, dim3(nb), dim3(BG_T), 0, st, src, (const uint32_t *) koff, flt, d_events, capacity, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("scan, write");
    if ((rc = fetch())) return fail(rc);
    if (W.bad_table || W.n_slots != src.n_slots) {
        ctx->last_error = "bag ingest: the message table does not fit the file (" + std::to_string(W.bad_table) + " messages outside it, " +
                          std::to_string(W.n_slots) + " events)";
        return fail(ECAL_ERR_INVALID);
    }
    I.n_events = W.n_events;
    I.n_outside = W.n_outside;
    I.n_negative = W.n_negative;
    I.n_before_start = W.n_before_start;
    // every event in front of the offender has one of the four classes
    I.n_after_end = W.first_stop == BG_NONE ? 0 : I.n_raw_events - (W.n_events + W.n_outside + W.n_negative + W.n_before_start);
    if (I.n_events > capacity) {
        ctx->last_error = "bag ingest: " + std::to_string(I.n_events) + " records, more than the capacity";
        return fail(ECAL_ERR_RANGE);
    }
    return ECAL_OK;
}

// Bytes of a file through a small read-ahead window: the walk asks for a record's header length, its header, the front of a message
// — a few dozen bytes at places 10 – 100 KB apart — and one pread of a window serves them all.
struct BagFileReader {
    int fd;
    uint64_t file_bytes;
    std::vector<uint8_t> win;
    uint64_t win_at = 0, win_n = 0;
    static constexpr size_t WINDOW = 512;
    bool pread_all(void *dst, size_t n, uint64_t at) const {
        for (size_t got = 0; got < n;) {
            const ssize_t rd = pread(fd, (uint8_t *) dst + got, n - got, (off_t) (at + got));
            if (rd <= 0) return false;
            got += (size_t) rd;
        }
        return true;
    }
    bool operator()(uint64_t pos, uint8_t *dst, size_t n) {
        if (pos >= win_at && pos + n <= win_at + win_n) {
            memcpy(dst, win.data() + (pos - win_at), n);
            return true;
        }
        if (n >= WINDOW) return pread_all(dst, n, pos);
        const size_t want = (size_t) std::min<uint64_t>(WINDOW, file_bytes - pos);
        win.resize(WINDOW);
        if (!pread_all(win.data(), want, pos)) return false;
        win_at = pos;
        win_n = want;
        memcpy(dst, win.data(), n);
        return true;
    }
};

// file -> (message table on the host, from record headers, beside the upload) -> file in HBM -> records in a device buffer of their
// own (null for none), the file's bytes freed
int bag_file_to_events(ecal_ctx *ctx, const char *path, const ecal_bag_options *opt, uint8_t **d_events, ecal_bag_info &I) {
    *d_events = nullptr;
    ecal_bag_options o;
    if (opt) o = *opt; else ecal_bag_default_options(&o);
    int rc = bag_check_options(ctx, o);
    if (rc) return rc;
    const BagChoice choice = bag_choice(&o);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        ctx->last_error = std::string("bag ingest: cannot open ") + path;
        return ECAL_ERR_INVALID;
    }
    struct stat sb;
    if (fstat(fd, &sb) != 0) {
        close(fd);
        ctx->last_error = std::string("bag ingest: cannot read ") + path;
        return ECAL_ERR_INVALID;
    }
    {   // the first line in front of everything: a file of another kind is not uploaded
        uint8_t head[32];
        BagFileReader rd{fd, (uint64_t) sb.st_size};
        const size_t hn = (size_t) std::min<uint64_t>((uint64_t) sb.st_size, sizeof(head));
        std::string err = "cannot be read";
        if ((hn && !rd.pread_all(head, hn, 0)) || bag_check_magic(head, hn, &err)) {
            close(fd);
            ctx->last_error = "bag ingest: " + err + " (" + path + ")";
            return ECAL_ERR_INVALID;
        }
    }
    std::vector<BagMessage> table;
    BagCounts c;
    memset(&c, 0, sizeof(c));
    ecal_ingest_upload up;
    rc = ecal_ingest_upload_indexed(ctx, "bag", "bag ingest", "host message index", path, fd, 0, (uint64_t) sb.st_size, [&](std::string *error, const void **tab, size_t *tab_bytes) {
        BagFileReader rd{fd, (uint64_t) sb.st_size};
        std::string err;
        const int index_rc = bag_walk(rd, (uint64_t) sb.st_size, choice, c, [&](const BagMessage &m) { table.push_back(m); }, &err);
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
    const size_t o_words = up16((size_t) (n_messages + 1) * 8);
    if ((rc = ecal_ensure(ctx, buf, o_words + sizeof(BagWords)))) return rc;
    BagWords *d_w = (BagWords *) (buf.as<uint8_t>() + o_words);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(BagWords), &d_w->first_stop, st))) return rc;
    hipLaunchKernelGGL(bag_message_scan_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<const BagMessage *>(d_messages), (uint32_t) n_messages,
                       n_bytes, buf.as<unsigned long long>(), d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    BagWords W;
    if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return rc;
    if (W.bad_table) {
        ctx->last_error = "bag ingest: " + std::to_string(W.bad_table) + " messages of the table do not lie within the file";
        return ECAL_ERR_INVALID;
    }
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
