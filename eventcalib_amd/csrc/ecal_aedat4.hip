// AEDAT 4 ingest (include/ecal.h, "aedat4 ingest"): an iniVation DV recording resident in HBM — a chain of packets, each one LZ4 frame
// around a FlatBuffer of 16-byte events — into packed 25-byte records.  The header parser, the chain walk, the LZ4 frame walker, the
// FlatBuffer locator, the event and the filter are aedat4_events.hpp's (shared with the host decoder and the CPU test);
// design/18_aedat4_ingest.md has the reasoning.
//
// The chain is NOT walked here (a packet is found only through the header before it): the host indexes the packets of the event
// stream (ecal_aedat4_index_packets) and the table comes in with the file.  Launches, with NO waiting between workgroups — state
// crosses workgroups only between launches, or inside the one-workgroup scans:
//   LZ4  1. aedat4_frame_kernel<false>  one wave a packet: the frame walked without producing a byte, everything validated, the
//                                       inflated size written; the first bad packet through one 64-bit atomic minimum
//        2. aedat4_span_scan_kernel     one workgroup: the sizes, each padded to 16 bytes, scanned into spans of the scratch.  The host
//                                       reads the total (the one extra synchronisation) and sizes the scratch
//        3. aedat4_frame_kernel<true>   one wave a packet: the same walk, the lanes sharing every literal and match copy; the last
//                                       64 KiB of output live in an LDS ring, which is what a match reads
//   both 4. aedat4_locate_kernel        a thread a packet: the FlatBuffer read, {byte offset of the first event, count} written
//        5. aedat4_packet_scan_kernel   one workgroup: the counts scanned into an event-slot space
//        6. aedat4_verdict_kernel       every slot classed; the kept events per block; the first slot that reaches end_time
//        7. ecal_scan_blocks            the blocks' first kept index
//        8. aedat4_write_kernel         classed again; the kept events below the first offender packed into LDS and copied out
// Compression NONE skips 1 - 3 and locates in the file itself.
// The bodies of passes 6 and 8 are slot_kernels.hpp's (A4Format below is this format's policy), the table scans, the bisection, the
// clipped load and the tails of passes 6 and 8 ingest_blocks.hpp's, the host side of passes 6 - 8 ingest_driver.hpp's
// (ecal_ingest_verdict_write), all shared with the other table ingests; the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "slot_kernels.hpp"
#include "ingest_driver.hpp"
#include "aedat4_events.hpp"

namespace ecal {

using namespace ecal_aedat4;

static_assert(ECAL_AEDAT4_NONE == A4_COMP_NONE && ECAL_AEDAT4_LZ4 == A4_COMP_LZ4 && ECAL_AEDAT4_LZ4_HIGH == A4_COMP_LZ4_HIGH &&
                  ECAL_AEDAT4_ZSTD == A4_COMP_ZSTD && ECAL_AEDAT4_ZSTD_HIGH == A4_COMP_ZSTD_HIGH, "compression codes");
static_assert(ECAL_ERR_INVALID == A4_INVALID && ECAL_ERR_RANGE == A4_RANGE && ECAL_OK == A4_OK, "status codes");
static_assert(sizeof(ecal_aedat4_packet) == 16 && sizeof(A4Packet) == 16, "packet table entry");

constexpr int A4_T = A4_BLOCK_THREADS;
constexpr uint32_t A4_PER = A4_THREAD_EVENTS;
constexpr uint32_t A4_BLOCK = A4_BLOCK_EVENTS;   // slots per block, and records staged in LDS (25 600 bytes)
constexpr unsigned long long A4_NONE = ~0ull;
constexpr uint32_t A4_RING = 65536;              // the LDS window of the inflate pass: a match reaches back 65 535 bytes at most
constexpr uint32_t A4_STAGE = 1024;              // compressed bytes staged in LDS in front of the token walk

// the counters of one ingest (device)
struct A4Words {
    unsigned long long n_slots;          // events of the located table
    unsigned long long first_stop;       // the first slot that reaches end_time (A4_NONE: none)
    unsigned long long n_events, n_outside, n_negative, n_before_start;
    unsigned long long bad_packet;       // (index << 8 | why) of the first packet refused (A4_NONE: none)
    unsigned long long n_inflated, span_total, n_compressed;
};

__device__ __forceinline__ void a4_refuse(A4Words *w, uint32_t k, int why) { atomicMin(&w->bad_packet, ((unsigned long long) k << 8) | (unsigned long long) why); }

// The packet's data read through a window of LDS: the token walk's dependent loads are LDS loads; a refill is 16 loads in flight at
// once.  Every lane of the wave asks for the same byte, so the refill's barriers are reached by all of them.  Nothing at or behind n
// is loaded.
struct A4StagedReader {
    const uint8_t *g;
    uint64_t n;
    uint8_t *s_in;
    mutable uint64_t win0;
    __device__ __forceinline__ uint8_t operator()(uint64_t i) const {
        if (i - win0 >= A4_STAGE) {   // (also win0 > i)
            __syncthreads();
            win0 = i;
#pragma unroll
            for (uint32_t j = 0; j < A4_STAGE / 64; j++) {
                const uint64_t a = i + threadIdx.x + 64u * j;
                s_in[threadIdx.x + 64u * j] = a < n ? g[a] : (uint8_t) 0;
            }
            __syncthreads();
        }
        return s_in[i - win0];
    }
};

// The wave's share of every copy.  out[0, limit): the packet's span of the scratch — nothing is stored outside it, nothing at or
// behind n of the packet's data is loaded (the size pass has made both impossible; the clamps stand all the same).  ring: the last
// A4_RING bytes of output, byte q at ring[q mod A4_RING].  A match is read from the ring alone, never from global memory: the
// workgroup is this one wave, and a barrier stands between every store to the ring and every load that may name its byte.
struct A4WaveSink {
    const uint8_t *g;
    uint64_t n;
    uint8_t *out;
    uint64_t limit;
    uint8_t *ring;
    uint64_t p;
    __device__ __forceinline__ void put(uint64_t q, uint8_t b) {
        ring[q & (A4_RING - 1u)] = b;
        if (q < limit) out[q] = b;
    }
    __device__ __forceinline__ void literals(uint64_t i, uint64_t len) {
        for (uint64_t k = threadIdx.x; k < len; k += 64u) put(p + k, i + k < n ? g[i + k] : (uint8_t) 0);
        p += len;
        __syncthreads();
    }
    __device__ __forceinline__ void match(uint32_t off, uint64_t len) {
        if (off >= 64u) {
            // 64 bytes a step: their sources lie off >= 64 bytes back, so every one was stored in an earlier step or before the match.
            // A store of this step may land on the ring slot of another lane's source (off close to A4_RING): the barrier between
            // the loads and the stores keeps the old byte
            for (uint64_t k0 = 0; k0 < len; k0 += 64u) {
                const uint64_t k = k0 + threadIdx.x;
                uint8_t b = 0;
                if (k < len) b = ring[(p + k - off) & (A4_RING - 1u)];
                __syncthreads();
                if (k < len) put(p + k, b);
                __syncthreads();
            }
        } else {
            // a short period: byte k is the byte at match start + k mod off.  The off bytes in front of the match go into registers
            // once (lane j < off holds byte j of the period) and every step takes its bytes from there
            const int pat = ring[(p - off + (threadIdx.x % off)) & (A4_RING - 1u)];
            for (uint64_t k0 = 0; k0 < len; k0 += 64u) {
                const uint64_t k = k0 + threadIdx.x;
                const int b = __shfl(pat, (int) (k % off), 64);
                if (k < len) put(p + k, (uint8_t) b);
            }
            __syncthreads();
        }
        p += len;
    }
};

// One wave a packet.  PRODUCE = false: the size pass (sizes[k] = the inflated size, or 0 with the packet refused).  PRODUCE = true:
// the inflate pass into scratch + span[k], at most sizes[k] bytes.
template <bool PRODUCE>
__global__ __launch_bounds__(64) void aedat4_frame_kernel(const uint8_t *__restrict__ file, uint64_t n_bytes, const A4Packet *__restrict__ packets,
                                                          uint32_t n_packets, unsigned long long *__restrict__ sizes,
                                                          const unsigned long long *__restrict__ span, uint8_t *__restrict__ scratch,
                                                          uint64_t scratch_bytes, A4Words *__restrict__ w) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[A4_STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[PRODUCE ? A4_RING : 16];
    const uint32_t k = blockIdx.x;
    if (k >= n_packets) return;
    const uint64_t off = packets[k].offset, len = packets[k].n_bytes;
    if (off > n_bytes || len > n_bytes - off) {   // (the same for every lane)
        if (!PRODUCE && threadIdx.x == 0) {
            sizes[k] = 0;
            a4_refuse(w, k, A4E_TABLE_ENTRY);
        }
        return;
    }
    const A4StagedReader rd{file + off, len, s_in, ~0ull - A4_STAGE};
    uint64_t inflated = 0;
    if constexpr (PRODUCE) {
        uint64_t base = span[k], limit = sizes[k];
        if (base > scratch_bytes) base = scratch_bytes;
        if (limit > scratch_bytes - base) limit = scratch_bytes - base;
        A4WaveSink sink{file + off, len, scratch + base, limit, s_ring, 0};
        (void) a4_lz4_frame(rd, len, sink, &inflated);
    } else {
        (void) s_ring; (void) span; (void) scratch; (void) scratch_bytes;
        A4SizeSink sink;
        const int why = a4_lz4_frame(rd, len, sink, &inflated);
        if (threadIdx.x == 0) {
            sizes[k] = why ? 0ull : inflated;
            if (why) a4_refuse(w, k, why);
        }
    }
}

// span[k] = the padded sizes of the packets before k, span[n] = all of them (table_exscan_1024); the plain sum of the sizes.
// One workgroup.
__global__ __launch_bounds__(1024) void aedat4_span_scan_kernel(const unsigned long long *__restrict__ sizes, uint32_t n,
                                                                unsigned long long *__restrict__ span, A4Words *__restrict__ w) {
    __shared__ unsigned long long s_plain[16];
    unsigned long long plain = 0;
    for (uint64_t p = threadIdx.x; p < n; p += 1024u) plain += sizes[p];
    for (int d = 32; d > 0; d >>= 1) plain += __shfl_xor(plain, d, 64);
    if ((threadIdx.x & 63) == 0) s_plain[threadIdx.x >> 6] = plain;
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (sizes[p] + 15ull) & ~15ull; }, span);   // (its barrier orders s_plain too)
    if (threadIdx.x == 0) {
        unsigned long long ptot = 0;
        for (int x = 0; x < 16; x++) ptot += s_plain[x];
        w->span_total = tot;
        w->n_inflated = ptot;
    }
}

// a thread a packet: located[k] = {the first event's byte offset in `src` (the scratch, or the file itself with no compression), count}
__global__ __launch_bounds__(256) void aedat4_locate_kernel(const uint8_t *__restrict__ file, uint64_t n_bytes, const A4Packet *__restrict__ packets,
                                                            uint32_t n_packets, const unsigned long long *__restrict__ sizes,
                                                            const unsigned long long *__restrict__ span, const uint8_t *__restrict__ scratch,
                                                            uint64_t scratch_bytes, int lz4, A4Packet *__restrict__ located, A4Words *__restrict__ w) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_packets) return;
    const uint64_t off = packets[k].offset, len = packets[k].n_bytes;
    uint64_t base = off, have = len, first = 0;
    uint32_t count = 0;
    int why = A4E_NONE;
    const uint8_t *src = file;
    if (off > n_bytes || len > n_bytes - off) why = A4E_TABLE_ENTRY;
    else if (lz4) {
        base = span[k];
        have = sizes[k];
        src = scratch;
        if (base > scratch_bytes || have > scratch_bytes - base) why = A4E_TABLE_ENTRY;   // (cannot be: the spans are the scan of the sizes)
    }
    if (!why) why = a4_locate_events(src + base, have, &first, &count);
    if (why) {
        a4_refuse(w, k, why);
        count = 0;
    } else {
        atomicAdd(&w->n_compressed, (unsigned long long) len);
    }
    located[k] = A4Packet{base + first, count, 0u};
}

// first[p] = the events of the packets before p, first[n] = all of them (table_exscan_1024).  One workgroup.
__global__ __launch_bounds__(1024) void aedat4_packet_scan_kernel(const A4Packet *__restrict__ located, uint32_t n, unsigned long long *__restrict__ first,
                                                                  A4Words *__restrict__ w) {
    const unsigned long long tot = table_exscan_1024(n, [&](uint64_t p) { return (unsigned long long) located[p].n_bytes; }, first);
    if (threadIdx.x == 0) w->n_slots = tot;
}

struct A4Source {
    const uint8_t *src;              // the scratch, or the file
    uint64_t n_bytes;
    uint64_t n_slots;
    const A4Packet *located;         // {first event's byte offset in src, count}
    const unsigned long long *first; // [n_packets + 1]
    uint32_t n_packets;
};

// the thread's slots: the four words of every event
struct A4Slots {
    uint32_t w[A4_PER][4];
    uint32_t n;
    __device__ __forceinline__ A4Slots(const A4Source &s) {
        const uint64_t s0 = ((uint64_t) blockIdx.x * A4_T + threadIdx.x) * A4_PER;
        n = s0 < s.n_slots ? (uint32_t) (s.n_slots - s0 < A4_PER ? s.n_slots - s0 : A4_PER) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < A4_PER; j++) w[j][0] = w[j][1] = w[j][2] = w[j][3] = 0u;
        if (!n) return;
        const uint64_t b0 = (uint64_t) blockIdx.x * A4_BLOCK;
        const uint64_t b1 = b0 + A4_BLOCK < s.n_slots ? b0 + A4_BLOCK - 1u : s.n_slots - 1u;
        const uint32_t p_lo = table_find(s.first, 0u, s.n_packets - 1u, b0);
        const uint32_t p_hi = table_find(s.first, p_lo, s.n_packets - 1u, b1);
        uint32_t p = table_find(s.first, p_lo, p_hi, s0);
        uint64_t p_first = s.first[p], p_next = s.first[p + 1], p_off = s.located[p].offset;
#pragma unroll
        for (uint32_t j = 0; j < A4_PER; j++) {
            if (j < n) {
                const uint64_t slot = s0 + j;
                if (slot >= p_next) {   // (packets of no events in between are stepped over by the search)
                    p = table_find(s.first, p + 1u, p_hi, slot);
                    p_first = s.first[p];
                    p_next = s.first[p + 1];
                    p_off = s.located[p].offset;
                }
                // the event from aligned words, whatever its byte offset; an offset behind the buffer reads zeros
                const uint64_t off = p_off + (slot - p_first) * A4_EVENT_BYTES;
                if (off + A4_EVENT_BYTES <= s.n_bytes && off + A4_EVENT_BYTES > off) {
                    const uint64_t al = off & ~3ull;
                    const uint32_t sh = 8u * (uint32_t) (off & 3u);
                    uint32_t v[5];
#pragma unroll
                    for (uint32_t q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint32_t *>(s.src + al + 4u * q);
                    v[4] = sh ? load32_clipped(s.src, al + 16u, s.n_bytes) : 0u;
#pragma unroll
                    for (uint32_t q = 0; q < 4; q++) w[j][q] = (uint32_t) ((((uint64_t) v[q + 1] << 32) | v[q]) >> sh);
                }
            }
        }
    }
    __device__ __forceinline__ A4Event event(uint32_t j) const { return a4_event(w[j][0], w[j][1], w[j][2], w[j][3]); }
};

// the format of slot_kernels.hpp's bodies
struct A4Format {
    typedef A4Source Source;
    typedef A4Filter Filter;
    typedef A4Words Words;
    typedef A4Slots Slots;
    static constexpr int T = A4_T, N_DROPS = 3;
    static constexpr uint32_t PER = A4_PER, BLOCK = A4_BLOCK;
    static constexpr uint8_t KEEP = A4_CLASS_KEEP, STOP = A4_CLASS_STOP;
    static __device__ __forceinline__ Slots slots(const Source &src, unsigned long long *) { return Slots(src); }
    static __device__ __forceinline__ bool is_event(const Slots &, uint32_t) { return true; }
    static __device__ __forceinline__ uint8_t classify(const Slots &s, uint32_t j, const Filter &flt, double *t, uint32_t *x, uint32_t *y) {
        return a4_classify(s.event(j), flt, t, x, y);
    }
    static __device__ __forceinline__ uint8_t polarity(const Slots &s, uint32_t j) { return s.event(j).on; }
    static __device__ __forceinline__ constexpr uint8_t drop_class(int i) { return i == 0 ? A4_CLASS_OUTSIDE : i == 1 ? A4_CLASS_NEGATIVE : A4_CLASS_BEFORE_START; }
    static __device__ __forceinline__ unsigned long long *drop_counter(Words *w, int i) { return i == 0 ? &w->n_outside : i == 1 ? &w->n_negative : &w->n_before_start; }
};

__global__ __launch_bounds__(A4_T) void aedat4_verdict_kernel(A4Source src, A4Filter flt, uint32_t *__restrict__ blk_keep, A4Words *__restrict__ w) {
    slot_verdict_body<A4Format>(src, flt, blk_keep, w);
}

__global__ __launch_bounds__(A4_T) void aedat4_write_kernel(A4Source src, const uint32_t *__restrict__ blk_koff, A4Filter flt,
                                                            uint8_t *__restrict__ events, uint64_t capacity, A4Words *__restrict__ w) {
    slot_write_body<A4Format>(src, blk_koff, flt, events, capacity, w);
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_aedat4_default_options(ecal_aedat4_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->compression = ECAL_AEDAT4_LZ4;
    opt->stream_id = -1;
    opt->auto_time_base = 1;
    opt->start_time = -INFINITY;
    opt->max_inflated_bytes = A4_DEFAULT_MAX_INFLATED;
}

extern "C" uint32_t ecal_aedat4_block_events(void) { return A4_BLOCK; }

namespace {

void a4_info_from_counts(ecal_aedat4_info &I, const A4Counts &c) {
    I.n_packets = c.n_packets;
    I.n_other_packets = c.n_other_packets;
    I.n_trailing_bytes = c.n_trailing_bytes;
    I.n_compressed_bytes = c.n_compressed_bytes;
    I.first_stamp_us = c.first_stamp_us;
    I.compression = c.compression;
    I.stream_id = c.stream_id;
}

int a4_check_args(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const void *d_packets, uint64_t n_packets, int compression) {
    if (compression != ECAL_AEDAT4_NONE && compression != ECAL_AEDAT4_LZ4 && compression != ECAL_AEDAT4_LZ4_HIGH) {
        ctx->last_error = "AEDAT 4 ingest: the compression must be given: ECAL_AEDAT4_NONE or ECAL_AEDAT4_LZ4";
        return ECAL_ERR_INVALID;
    }
    const int rc = ecal_ingest_check_buffer(ctx, "AEDAT 4 ingest", d_file, n_bytes, 16, "file");
    return rc ? rc : ecal_ingest_check_buffer(ctx, "AEDAT 4 ingest", d_packets, n_packets, 8, "packet table", nullptr, "packets");
}

int a4_check_options(ecal_ctx *ctx, const ecal_aedat4_options &o) {
    if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) {
        ctx->last_error = "AEDAT 4 ingest: flip_x / flip_y need width / height";
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

// count_only: *n_count = the events before any drop, nothing else is written.
// own_events != null: the records go into a buffer allocated here for the count (the caller's to hipFree, null when there is nothing
// to free); else into d_events / capacity
int a4_ingest(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const A4Packet *d_packets, uint64_t n_packets, int compression,
              const ecal_aedat4_options &o, uint8_t *d_events, uint64_t capacity, uint8_t **own_events, bool count_only, uint64_t *n_count,
              ecal_aedat4_info &I, hipStream_t st) {
    const bool lz4 = compression != ECAL_AEDAT4_NONE;
    I.compression = compression;
    I.n_packets = n_packets;
    I.time_base = o.time_base;
    if (own_events) *own_events = nullptr;
    if (n_count) *n_count = 0;
    if (!n_packets) return ECAL_OK;
    const uint32_t n = (uint32_t) n_packets;
    ecal_load_timer tm("aedat4", ctx->sw.load_trace, st);
    const size_t o_sizes = 0, o_span = o_sizes + up16((size_t) n * 8), o_loc = o_span + up16(((size_t) n + 1) * 8),
                 o_first = o_loc + up16((size_t) n * 16), o_words = o_first + up16(((size_t) n + 1) * 8), total = o_words + sizeof(A4Words);
    int rc;
    if ((rc = ecal_ensure(ctx, ctx->aedat4_tables, total))) return rc;
    uint8_t *base = ctx->aedat4_tables.as<uint8_t>();
    unsigned long long *sizes = (unsigned long long *) (base + o_sizes), *span = (unsigned long long *) (base + o_span),
                       *first = (unsigned long long *) (base + o_first);
    A4Packet *located = (A4Packet *) (base + o_loc);
    A4Words *d_w = (A4Words *) (base + o_words);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(A4Words), &d_w->first_stop, st))) return rc;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(&d_w->bad_packet, 0xFF, sizeof(unsigned long long), st));
    tm.mark("start");
    A4Words W;
    auto fetch = [&]() { return ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st); };
    auto launched = [&]() -> int {
        ECAL_HIP_TRY(ctx, hipGetLastError());
        return ECAL_OK;
    };
    // the first refused packet by name: its data's offset is the table's (read back: one entry)
    auto refused = [&]() -> int {
        const uint64_t k = W.bad_packet >> 8;
        A4Packet p{0, 0, 0};
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(&p, d_packets + k, sizeof(p), hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
        ctx->last_error = a4_name_packet(k, p.offset) + a4_why((int) (W.bad_packet & 0xFFu));
        return ECAL_ERR_INVALID;
    };
    uint8_t *scratch = nullptr;
    uint64_t scratch_bytes = 0;
    if (lz4) {
        hipLaunchKernelGGL(aedat4_frame_kernel<false>, dim3(n), dim3(64), 0, st, d_file, n_bytes, d_packets, n, sizes,
                           (const unsigned long long *) nullptr, (uint8_t *) nullptr, (uint64_t) 0, d_w);
        if ((rc = launched())) return rc;
        tm.mark("size pass");
        hipLaunchKernelGGL(aedat4_span_scan_kernel, dim3(1), dim3(1024), 0, st, (const unsigned long long *) sizes, n, span, d_w);
        if ((rc = launched())) return rc;
        if ((rc = fetch())) return rc;   // the one look that sizes the scratch
        tm.mark("span scan");
        if (W.bad_packet != A4_NONE) return refused();
        I.n_inflated_bytes = W.n_inflated;
        if (W.n_inflated > o.max_inflated_bytes) {
            ctx->last_error = "AEDAT 4 ingest: the packets inflate to " + std::to_string(W.n_inflated) + " bytes, more than max_inflated_bytes (" +
                              std::to_string(o.max_inflated_bytes) + ")";
            return ECAL_ERR_RANGE;
        }
        scratch_bytes = W.span_total;
        if ((rc = ecal_ensure(ctx, ctx->aedat4_inflated, (size_t) scratch_bytes + 16))) return rc;
        scratch = ctx->aedat4_inflated.as<uint8_t>();
        hipLaunchKernelGGL(aedat4_frame_kernel<true>, dim3(n), dim3(64), 0, st, d_file, n_bytes, d_packets, n, sizes,
                           (const unsigned long long *) span, scratch, scratch_bytes, d_w);
        if ((rc = launched())) return rc;
        tm.mark("inflate pass");
    }
    hipLaunchKernelGGL(aedat4_locate_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_file, n_bytes, d_packets, n, (const unsigned long long *) sizes,
                       (const unsigned long long *) span, (const uint8_t *) scratch, scratch_bytes, lz4 ? 1 : 0, located, d_w);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(aedat4_packet_scan_kernel, dim3(1), dim3(1024), 0, st, (const A4Packet *) located, n, first, d_w);
    if ((rc = launched())) return rc;
    if ((rc = fetch())) return rc;   // the grid is a count of the table
    tm.mark("locate, packet scan");
    if (W.bad_packet != A4_NONE) return refused();
    I.n_compressed_bytes = W.n_compressed;
    if (!lz4) {
        I.n_inflated_bytes = W.n_compressed;
        if (I.n_inflated_bytes > o.max_inflated_bytes) {
            ctx->last_error = "AEDAT 4 ingest: the packets hold " + std::to_string(I.n_inflated_bytes) + " bytes, more than max_inflated_bytes (" +
                              std::to_string(o.max_inflated_bytes) + ")";
            return ECAL_ERR_RANGE;
        }
    }
    I.n_raw_events = W.n_slots;
    if (W.n_slots > 0xFFFFFFFFull) {
        I.n_events = W.n_slots;
        ctx->last_error = "AEDAT 4 ingest: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    if (n_count) *n_count = W.n_slots;
    if (count_only || !W.n_slots) return ECAL_OK;
    const uint32_t nb = (uint32_t) ((W.n_slots + A4_BLOCK - 1) / A4_BLOCK);
    if ((rc = ecal_ensure(ctx, ctx->aedat4_blocks, 2 * up16(((size_t) nb + 1) * 4)))) return rc;
    uint32_t *keep = ctx->aedat4_blocks.as<uint32_t>(), *koff = keep + up16(((size_t) nb + 1) * 4) / 4;
    if (own_events) {
        capacity = W.n_slots;
        if ((rc = ecal_ingest_alloc_records(ctx, "AEDAT 4 ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    const A4Filter flt{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
    const A4Source src{lz4 ? scratch : d_file, lz4 ? scratch_bytes : n_bytes, W.n_slots, located, first, n};
    return ecal_ingest_verdict_write(
        ctx, "AEDAT 4 ingest", tm, nb, keep, koff, (const A4Words *) d_w, capacity, own_events, I, st,
        [&] { hipLaunchKernelGGL(aedat4_verdict_kernel, dim3(nb), dim3(A4_T), 0, st, src, flt, keep, d_w); },
        [&] { hipLaunchKernelGGL(aedat4_write_kernel, dim3(nb), dim3(A4_T), 0, st, src, (const uint32_t *) koff, flt, d_events, capacity, d_w); },
        [](const A4Words &, uint64_t *) { return ECAL_OK; });
}

// file -> header on the host -> (the packet headers read and the stream chosen on a host thread, beside the upload) -> the file in HBM
// -> records in a device buffer of their own (null for none), the file's bytes freed
int a4_file_to_events(ecal_ctx *ctx, const char *path, const ecal_aedat4_options *opt, uint8_t **d_events, ecal_aedat4_info &I) {
    *d_events = nullptr;
    ecal_aedat4_options o;
    if (opt) o = *opt; else ecal_aedat4_default_options(&o);
    int rc = a4_check_options(ctx, o);
    if (rc) return rc;
    int fd;
    uint64_t file_bytes;
    std::vector<uint8_t> head;
    if ((rc = ecal_ingest_open_head(ctx, "AEDAT 4 ingest", path, A4_HEADER_LIMIT, nullptr, &fd, &file_bytes, &head))) return rc;
    A4Header h;
    std::string err;
    uint64_t end = 0;
    rc = a4_parse_header(head.data(), head.size(), head.size() == file_bytes, &h, &err);
    if (!rc) rc = a4_packets_end(h, file_bytes, &end, &err);
    if (rc) {
        close(fd);
        ctx->last_error = err + " (" + path + ")";
        return rc;
    }
    std::vector<A4Packet> table;
    A4Counts c;
    memset(&c, 0, sizeof(c));
    c.compression = h.compression;
    ecal_ingest_upload up;
    rc = ecal_ingest_upload_indexed(ctx, "aedat4", "AEDAT 4 ingest", "host packet index", path, fd, 0, ECAL_INGEST_ANY_SIZE, [&](std::string *error, const void **tab, size_t *tab_bytes) {
        std::vector<A4ChainPacket> chain;
        int index_rc = a4_walk_chain([&](uint64_t pos, uint8_t *raw) { return ecal_ingest_pread_all(fd, raw, 8, pos); }, h.packets_begin, end,
                                     [&](const A4ChainPacket &p) { chain.push_back(p); }, &c.n_trailing_bytes, error);
        if (!index_rc)
            index_rc = a4_choose_stream(chain, h.compression, o.stream_id, [&](uint64_t off, uint32_t nb, std::vector<uint8_t> &out) {
                out.resize(nb);
                return nb == 0 || ecal_ingest_pread_all(fd, out.data(), nb, off);
            }, table, c, error);
        if (index_rc) *error += std::string(" (") + path + ")";
        *tab = table.data();
        *tab_bytes = table.size() * sizeof(A4Packet);
        return index_rc;
    }, &up);
    if (rc) return rc;
    a4_info_from_counts(I, c);
    if (o.auto_time_base) o.time_base = c.first_stamp_us;
    I.time_base = o.time_base;
    ecal_aedat4_info K = I;
    rc = a4_ingest(ctx, up.d_file, up.n_bytes, (const A4Packet *) up.d_table, table.size(), h.compression, o, nullptr, 0, d_events, false, nullptr, K,
                   ctx->stream);
    I.n_raw_events = K.n_raw_events;
    I.n_events = K.n_events;
    I.n_outside = K.n_outside;
    I.n_negative = K.n_negative;
    I.n_before_start = K.n_before_start;
    I.n_after_end = K.n_after_end;
    I.n_inflated_bytes = K.n_inflated_bytes;
    ecal_ingest_free_upload(ctx, &up);
    return rc;
}

}  // namespace

extern "C" int ecal_aedat4_parse_header(ecal_ctx *ctx, const uint8_t *data, uint64_t n_bytes, uint64_t file_bytes, int *compression,
                                        uint64_t *packets_begin, uint64_t *packets_end) {
    if (!compression || !packets_begin || !packets_end || (n_bytes && !data)) return ECAL_ERR_INVALID;
    A4Header h;
    std::string err;
    uint64_t end = 0;
    static const uint8_t none = 0;
    int rc = a4_parse_header(n_bytes ? data : &none, n_bytes, n_bytes >= file_bytes, &h, &err);
    if (!rc) rc = a4_packets_end(h, file_bytes, &end, &err);
    if (rc && ctx) ctx->last_error = "ecal_aedat4_parse_header: " + err;
    if (rc) return rc;
    *compression = h.compression;
    *packets_begin = h.packets_begin;
    *packets_end = end;
    return ECAL_OK;
}

extern "C" int ecal_aedat4_index_packets(ecal_ctx *ctx, const uint8_t *file_host, uint64_t n_bytes, int stream_id, ecal_aedat4_packet *out,
                                         uint64_t capacity, uint64_t *n_packets, ecal_aedat4_info *info) {
    if (!n_packets || (n_bytes && !file_host) || (capacity && !out)) return ECAL_ERR_INVALID;
    *n_packets = 0;
    std::vector<A4Packet> table;
    A4Counts c;
    std::string err;
    static const uint8_t none = 0;
    const int rc = a4_index_file_memory(n_bytes ? file_host : &none, n_bytes, stream_id, table, c, &err);
    if (rc) {
        if (ctx) ctx->last_error = "ecal_aedat4_index_packets: " + err;
        return rc;
    }
    *n_packets = table.size();
    for (size_t k = 0; k < table.size() && k < capacity; k++) memcpy(&out[k], &table[k], sizeof(A4Packet));
    if (info) {
        memset(info, 0, sizeof(*info));
        a4_info_from_counts(*info, c);
    }
    if (table.size() > capacity) {
        if (ctx) ctx->last_error = "ecal_aedat4_index_packets: " + std::to_string(table.size()) + " event packets, more than the capacity of the table";
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

extern "C" int ecal_aedat4_count_events_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_aedat4_packet *d_packets,
                                            uint64_t n_packets, const ecal_aedat4_options *opt, uint64_t *n_events, void *stream) {
    if (!ctx || !n_events || !opt) return ECAL_ERR_INVALID;
    *n_events = 0;
    int rc = a4_check_args(ctx, d_file, n_bytes, d_packets, n_packets, opt->compression);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ecal_aedat4_info I;
    memset(&I, 0, sizeof(I));
    return a4_ingest(ctx, d_file, n_bytes, reinterpret_cast<const A4Packet *>(d_packets), n_packets, opt->compression, *opt, nullptr, 0, nullptr, true,
                     n_events, I, (hipStream_t) stream);
}

extern "C" int ecal_events_from_aedat4_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_aedat4_packet *d_packets,
                                           uint64_t n_packets, const ecal_aedat4_options *opt, uint8_t *d_events, uint64_t capacity,
                                           ecal_aedat4_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_aedat4");
    if (!ctx || !opt) return ECAL_ERR_INVALID;
    ecal_aedat4_info I;
    memset(&I, 0, sizeof(I));
    I.stream_id = -1;
    if (info) *info = I;
    int rc = a4_check_args(ctx, d_file, n_bytes, d_packets, n_packets, opt->compression);
    if (rc) return rc;
    if ((rc = a4_check_options(ctx, *opt))) return rc;
    if (opt->auto_time_base) {
        ctx->last_error = "AEDAT 4 ingest: the _dev form takes an explicit time base (auto_time_base = 0)";
        return ECAL_ERR_INVALID;
    }
    if (capacity && !d_events) {
        ctx->last_error = "AEDAT 4 ingest: null record buffer";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = a4_ingest(ctx, d_file, n_bytes, reinterpret_cast<const A4Packet *>(d_packets), n_packets, opt->compression, *opt, d_events, capacity, nullptr,
                   false, nullptr, I, (hipStream_t) stream);
    if (info) *info = I;
    return rc;
}

extern "C" int ecal_stream_create_from_aedat4_file(ecal_ctx *ctx, const char *path, const ecal_aedat4_options *opt, ecal_stream **out,
                                                   ecal_aedat4_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_aedat4_info I;
    memset(&I, 0, sizeof(I));
    I.stream_id = -1;
    const int rc = a4_file_to_events(ctx, path, opt, &d_events, I);
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_aedat4_file", d_events, I.n_events, out);
}

extern "C" int ecal_aedat4_to_bin_file(ecal_ctx *ctx, const char *aedat4_path, const char *bin_path, const ecal_aedat4_options *opt,
                                       ecal_aedat4_info *info) {
    if (!ctx || !aedat4_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_aedat4_info I;
    memset(&I, 0, sizeof(I));
    I.stream_id = -1;
    const int rc = a4_file_to_events(ctx, aedat4_path, opt, &d_events, I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_aedat4_to_bin_file", d_events, I.n_events, bin_path);
}
