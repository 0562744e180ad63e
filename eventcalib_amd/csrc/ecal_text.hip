// Text ingest (include/ecal.h, "text ingest"): a text event file — lines of "stamp x y polarity", the input of the reference's
// EventStream::txt2bin (event/src/EventStream.cpp:25-67) — resident in HBM as one byte buffer, into packed 25-byte records.
// The line grammar, the number conversion and the filter are text_events.hpp's (shared with the host fallback and the CPU test).
//
// Launches, all over 64-bit byte offsets and with NO waiting between workgroups:
//   line index   1. text_count_kernel    '\n' per workgroup span of TX_SPAN bytes: one 128-bit load and a per-byte compare per
//                                        thread, the bytes of a last partial word one by one (nothing behind the text is read)
//                2. the exclusive scan of the spans' counts by one workgroup (ecal_scan_blocks, the association's)
//                3. text_offsets_kernel  line_off[k] = byte offset of line k; line_off[n_lines] closes the last line
//   parse        4. text_parse_kernel    one thread per line through text_parse_line into stamp / x / y / p / status; the first
//                                        malformed line, the first line with stamp > end_stamp, the first and the last record line
//                                        as minima / maxima (per wave, per workgroup, then one 64-bit atomic each), the lines for
//                                        the host in a compacted list
//   filter       5. text_verdict_kernel  the class of every line (text_classify; the base is read from the first record line's
//                                        stamp on the device), the kept lines per workgroup, the first line that meets end_time
//                6. ecal_scan_blocks
//                7. text_write_kernel    the kept lines below the first offender packed in LDS and copied to their final index
//                                        (aligned 32-bit stores), the duplicated last record, the totals
// Both "the stream ends here" rules are tests `line index < first offender`: a line behind the offender may be classed as kept by
// pass 5 and counted by pass 6 — that only moves offsets of lines that pass 7 drops anyway.
// The host sees the counters once, behind pass 7.  Only when the list of pass 4 is not empty it parses those lines (text and
// line table come down for that), patches the arrays with one small kernel and runs passes 5 - 7 again.
// The tail of pass 5 (kept count and first offender) and the copy-out of pass 7 are ingest_blocks.hpp's, shared with the other ingests;
// the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <chrono>
#include <algorithm>
#include <math.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <thread>
#include <atomic>
#include "ecal_ctx.hpp"
#include "block_utils.hpp"
#include "text_events.hpp"
#include "event_record.hpp"
#include "ingest_blocks.hpp"

namespace ecal {

using namespace ecal_text;

constexpr int TX_T = 256;                   // threads per workgroup, every kernel of this file
constexpr uint32_t TX_SPAN = TX_T * 16u;    // bytes per workgroup of the index passes: one 128-bit load per thread
constexpr unsigned long long TX_NONE = ~0ull;

// the counters of one ingest (device); the order is the layout the host's wipes rely on
struct TextWords {
    unsigned long long n_breaks;      // '\n' in front of the last byte: n_lines - 1
    unsigned long long first_bad, first_after, first_rec;   // minima of line indices (TX_NONE: none): malformed, stamp > end_stamp, record line
    unsigned long long last_rec_p1;   // 1 + the last record line (0: none)
    unsigned long long n_host, n_blank;
    unsigned long long first_stop;    // the first record that meets end_time (TX_NONE: none)
    unsigned long long n_events, n_negative, n_after_end, n_before_start;
    long long base;
};

// a line the host parsed, on its way into the arrays
struct TextPatch {
    int64_t stamp;
    double x, y;
    uint32_t line;
    uint8_t p, status;
};

// 0x80 in every byte of w that equals '\n' (exact per byte: no carries between bytes)
__device__ __forceinline__ uint32_t tx_newline_mask(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

__device__ __forceinline__ uint32_t tx_count16(const uint4 &w) {
    return (uint32_t) (__popc(tx_newline_mask(w.x)) + __popc(tx_newline_mask(w.y)) + __popc(tx_newline_mask(w.z)) +
                       __popc(tx_newline_mask(w.w)));
}

// '\n' among text[0, n_scan) per span; block_cnt may be null (ecal_text_count_lines_dev wants the total alone)
__global__ __launch_bounds__(TX_T) void text_count_kernel(const uint8_t *__restrict__ text, uint64_t n_scan, uint32_t *__restrict__ block_cnt,
                                                          TextWords *__restrict__ w) {
    __shared__ uint32_t s_red[TX_T / 64];
    const int tid = threadIdx.x;
    const uint64_t off = (uint64_t) blockIdx.x * TX_SPAN + (uint64_t) tid * 16u;
    uint32_t c = tx_count16(load16_clipped(text, off, n_scan));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t v = 0;
        for (int i = 0; i < TX_T / 64; i++) v += s_red[i];
        if (block_cnt) block_cnt[blockIdx.x] = v;
        if (v) atomicAdd(&w->n_breaks, (unsigned long long) v);
    }
}

// line_off[1 + rank of the '\n'] = the byte behind it; line_off[0] = 0; line_off[n_lines] = where a '\n' behind the last line
// would stand, plus one (so that every line is [line_off[k], line_off[k + 1] - 1))
__global__ __launch_bounds__(TX_T) void text_offsets_kernel(const uint8_t *__restrict__ text, uint64_t n_bytes, uint64_t n_scan,
                                                            const uint32_t *__restrict__ block_off, uint64_t n_lines,
                                                            uint64_t *__restrict__ line_off) {
    __shared__ unsigned long long s_red[TX_T / 64];
    const int tid = threadIdx.x;
    const uint64_t off = (uint64_t) blockIdx.x * TX_SPAN + (uint64_t) tid * 16u;
    const uint4 w = load16_clipped(text, off, n_scan);
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    uint32_t ex, eb, tot, tb;
    block_exscan_pair<TX_T>(tx_count16(w), 0u, s_red, &ex, &eb, &tot, &tb);
    uint64_t at = 1ull + block_off[blockIdx.x] + ex;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t b = (words[j >> 2] >> (8u * (j & 3u))) & 0xFFu;   // (bytes behind n_scan were loaded as zeros)
        if (b == '\n' && at < n_lines) line_off[at++] = off + j + 1u;
    }
    if (blockIdx.x == 0 && tid == 0) {
        line_off[0] = 0;
        line_off[n_lines] = n_bytes + (text[n_bytes - 1] == '\n' ? 0u : 1u);
    }
}

// minimum / maximum over the workgroup of up to five 32-bit candidates, then one 64-bit atomic per word that has one
__device__ __forceinline__ void tx_publish(uint32_t mn[3], uint32_t mx, uint32_t blanks, uint32_t (*s_red)[5], TextWords *w) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
        for (int i = 0; i < 3; i++) {
            const uint32_t v = __shfl_xor(mn[i], o, 64);
            mn[i] = v < mn[i] ? v : mn[i];
        }
        const uint32_t v = __shfl_xor(mx, o, 64);
        mx = v > mx ? v : mx;
        blanks += __shfl_xor(blanks, o, 64);
    }
    if ((tid & 63) == 0) {
        for (int i = 0; i < 3; i++) s_red[tid >> 6][i] = mn[i];
        s_red[tid >> 6][3] = mx;
        s_red[tid >> 6][4] = blanks;
    }
    __syncthreads();
    if (tid < 5) {
        uint32_t v = s_red[0][tid];
        for (int x = 1; x < TX_T / 64; x++) {
            const uint32_t o = s_red[x][tid];
            v = tid < 3 ? (o < v ? o : v) : tid == 3 ? (o > v ? o : v) : v + o;
        }
        if (tid == 0 && v != 0xFFFFFFFFu) atomicMin(&w->first_bad, (unsigned long long) v);
        if (tid == 1 && v != 0xFFFFFFFFu) atomicMin(&w->first_after, (unsigned long long) v);
        if (tid == 2 && v != 0xFFFFFFFFu) atomicMin(&w->first_rec, (unsigned long long) v);
        if (tid == 3 && v) atomicMax(&w->last_rec_p1, (unsigned long long) v);
        if (tid == 4 && v) atomicAdd(&w->n_blank, (unsigned long long) v);
    }
}

// one thread per line (n_lines < 2^32: line indices fit the 32-bit candidates, 0xFFFFFFFF = none)
__global__ __launch_bounds__(TX_T) void text_parse_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_off,
                                                          uint64_t n_lines, int has_end_stamp, int64_t end_stamp,
                                                          int64_t *__restrict__ stamp, double *__restrict__ x, double *__restrict__ y,
                                                          uint8_t *__restrict__ pol, uint8_t *__restrict__ status,
                                                          uint32_t *__restrict__ host_list, TextWords *__restrict__ w) {
    __shared__ uint32_t s_red[TX_T / 64][5];
    const uint64_t k = (uint64_t) blockIdx.x * TX_T + threadIdx.x;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx = 0, blanks = 0;
    if (k < n_lines) {
        const uint64_t b = line_off[k], e = line_off[k + 1] - 1u;
        const TextRecord r = text_parse_line(text + b, e - b);
        stamp[k] = r.stamp;
        x[k] = r.x;
        y[k] = r.y;
        pol[k] = r.p;
        status[k] = r.status;
        if (r.status == TEXT_MALFORMED) mn[0] = (uint32_t) k;
        if (r.status == TEXT_BLANK) blanks = 1;
        if (r.status == TEXT_OK) {
            if (has_end_stamp && r.stamp > end_stamp) mn[1] = (uint32_t) k;
            mn[2] = (uint32_t) k;
            mx = (uint32_t) k + 1u;
        }
        if (r.status == TEXT_NEEDS_HOST) host_list[atomicAdd(&w->n_host, 1ull)] = (uint32_t) k;   // (rare by design; at most n_lines entries)
    }
    tx_publish(mn, mx, blanks, s_red, w);
}

// the lines the host parsed, into the arrays and the counters
__global__ __launch_bounds__(TX_T) void text_patch_kernel(const TextPatch *__restrict__ patch, uint64_t n_patch, int has_end_stamp,
                                                          int64_t end_stamp, int64_t *__restrict__ stamp, double *__restrict__ x,
                                                          double *__restrict__ y, uint8_t *__restrict__ pol, uint8_t *__restrict__ status,
                                                          TextWords *__restrict__ w) {
    __shared__ uint32_t s_red[TX_T / 64][5];
    const uint64_t i = (uint64_t) blockIdx.x * TX_T + threadIdx.x;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx = 0, blanks = 0;
    if (i < n_patch) {
        const TextPatch q = patch[i];
        const uint32_t k = q.line;
        stamp[k] = q.stamp;
        x[k] = q.x;
        y[k] = q.y;
        pol[k] = q.p;
        status[k] = q.status;
        if (q.status == TEXT_MALFORMED) mn[0] = k;
        if (q.status == TEXT_BLANK) blanks = 1;
        if (q.status == TEXT_OK) {
            if (has_end_stamp && q.stamp > end_stamp) mn[1] = k;
            mn[2] = k;
            mx = k + 1u;
        }
    }
    tx_publish(mn, mx, blanks, s_red, w);
}

__device__ __forceinline__ int64_t tx_base(const ecal_text_options &o, const TextWords *w, const int64_t *stamp) {
    if (o.has_time_base) return o.time_base;
    const unsigned long long f = w->first_rec;
    return f == TX_NONE ? 0 : stamp[f];
}

// the class of every line, the kept lines per workgroup, the first record that meets end_time
__global__ __launch_bounds__(TX_T) void text_verdict_kernel(const int64_t *__restrict__ stamp, const uint8_t *__restrict__ status,
                                                            uint64_t n_lines, ecal_text_options o, uint8_t *__restrict__ cls,
                                                            uint32_t *__restrict__ block_cnt, TextWords *__restrict__ w) {
    const int tid = threadIdx.x;
    const uint64_t k = (uint64_t) blockIdx.x * TX_T + tid;
    const int64_t base = tx_base(o, w, stamp);
    const unsigned long long first_after = w->first_after;
    uint32_t keep = 0, stop = 0xFFFFFFFFu;
    if (k < n_lines) {
        uint8_t c = TEXT_CLASS_NONE;
        if (status[k] == TEXT_OK && k < first_after) {
            double t;
            c = text_classify(stamp[k], base, o.time_magnitude, o.start_time, o.has_end_time, o.end_time, &t);
            keep = c == TEXT_CLASS_KEEP ? 1u : 0u;
            if (c == TEXT_CLASS_STOP) stop = (uint32_t) k;
        }
        cls[k] = c;
    }
    block_keep_and_stop<TX_T>(keep, stop, block_cnt, &w->first_stop, [] { return 0ull; });   // (stop is a line index, not one within the block)
    if (blockIdx.x == 0 && tid == 0) w->base = base;
}

// the kept lines below the first offender, packed in LDS and copied out; the duplicated last record; the totals
__global__ __launch_bounds__(TX_T) void text_write_kernel(const uint8_t *__restrict__ text, uint64_t n_bytes, const int64_t *__restrict__ stamp,
                                                          const double *__restrict__ x, const double *__restrict__ y,
                                                          const uint8_t *__restrict__ pol, const uint8_t *__restrict__ status,
                                                          const uint8_t *__restrict__ cls, const uint32_t *__restrict__ block_off,
                                                          uint64_t n_lines, ecal_text_options o, uint8_t *__restrict__ events,
                                                          uint64_t capacity, TextWords *__restrict__ w) {
    __shared__ unsigned long long s_scan[TX_T / 64];
    __shared__ uint32_t s_cnt[TX_T / 64][3];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[TX_T * 25];
    const int tid = threadIdx.x;
    const uint64_t k = (uint64_t) blockIdx.x * TX_T + tid;
    const unsigned long long fa = w->first_after, fs = w->first_stop, X = fa < fs ? fa : fs;
    const int64_t base = w->base;
    const bool in = k < n_lines;
    const uint8_t st = in ? status[k] : (uint8_t) TEXT_BLANK, c = in ? cls[k] : (uint8_t) TEXT_CLASS_NONE;
    const bool below = k < X;
    const uint32_t keep = (in && below && c == TEXT_CLASS_KEEP) ? 1u : 0u;
    uint32_t cnt[3] = {(in && below && c == TEXT_CLASS_NEGATIVE) ? 1u : 0u, (in && !below && st == TEXT_OK) ? 1u : 0u,
                       (in && below && c == TEXT_CLASS_BEFORE_START) ? 1u : 0u};
    uint32_t ex, eb, tot, tb;
    block_exscan_pair<TX_T>(keep, 0u, s_scan, &ex, &eb, &tot, &tb);
    const uint64_t at0 = block_off[blockIdx.x];
    uint8_t rec[25];
    if (keep) {
        double t;
        (void) text_classify(stamp[k], base, o.time_magnitude, o.start_time, o.has_end_time, o.end_time, &t);
        pack_record(rec, t, x[k], y[k], pol[k]);
#pragma unroll
        for (int b = 0; b < 25; b++) s_rec[ex * 25u + b] = rec[b];
    }
    // the totals: the thread at the first offender knows the count in front of it; without an offender the thread of the last
    // line does, and the thread of the last record line appends the reference's duplicate
    if (in && X != TX_NONE && k == X) w->n_events = at0 + ex;
    if (in && X == TX_NONE) {
        const uint8_t last = text[n_bytes - 1];
        const bool ends_blank = last == '\n' || last == ' ' || last == '\t' || last == '\r';
        const unsigned long long L1 = w->last_rec_p1;
        const bool want_dup = o.duplicate_last && ends_blank && L1 != 0;
        if (k + 1 == n_lines) {
            const bool dup = want_dup && cls[L1 - 1] == TEXT_CLASS_KEEP;
            w->n_events = at0 + ex + keep + (dup ? 1u : 0u);
        }
        if (want_dup && k + 1 == L1 && keep) {
            const uint64_t at = at0 + ex + 1u;   // (no record line behind this one: the count so far is the total)
            if (at < capacity) {
#pragma unroll
                for (int b = 0; b < 25; b++) events[at * 25u + b] = rec[b];
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1)
        for (int i = 0; i < 3; i++) cnt[i] += __shfl_xor(cnt[i], d, 64);
    if ((tid & 63) == 0)
        for (int i = 0; i < 3; i++) s_cnt[tid >> 6][i] = cnt[i];
    __syncthreads();   // (... and s_rec)
    if (tid < 3) {
        uint32_t v = 0;
        for (int q = 0; q < TX_T / 64; q++) v += s_cnt[q][tid];
        if (v) atomicAdd(tid == 0 ? &w->n_negative : tid == 1 ? &w->n_after_end : &w->n_before_start, (unsigned long long) v);
    }
    block_copy_out<TX_T>(s_rec, tot, events, at0, capacity);
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_text_default_options(ecal_text_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->time_magnitude = 1e-6;
    opt->start_time = -INFINITY;
    opt->duplicate_last = 1;
}

namespace {

struct TextArrays {
    uint64_t *line_off;
    int64_t *stamp;
    double *x, *y;
    uint32_t *host_list, *cnt, *off;
    uint8_t *pol, *status, *cls;
};

size_t up8(size_t v) { return (v + 7) / 8 * 8; }

int text_count(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, ecal_devbuf &idx, TextWords *d_w, uint64_t *n_lines, uint32_t *nb_idx,
               bool want_blocks, hipStream_t st) {
    // a '\n' as the very last byte starts no line: the index passes look at the bytes in front of it
    const uint64_t n_scan = n_bytes - 1;
    const uint64_t nb64 = std::max<uint64_t>(1, (n_scan + TX_SPAN - 1) / TX_SPAN);
    if (nb64 > 0x7FFFFFFFull) {
        ctx->last_error = "text ingest: the text is too large for one launch";
        return ECAL_ERR_RANGE;
    }
    const uint32_t nb = (uint32_t) nb64;
    uint32_t *cnt = nullptr;
    if (want_blocks) {
        const int rc = ecal_ensure(ctx, idx, (2 * (size_t) nb + 1) * 4);
        if (rc) return rc;
        cnt = idx.as<uint32_t>();
    }
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_w, 0, sizeof(TextWords), st));
    ECAL_HIP_TRY(ctx, hipMemsetAsync(&d_w->first_bad, 0xFF, 3 * sizeof(unsigned long long), st));
    ECAL_HIP_TRY(ctx, hipMemsetAsync(&d_w->first_stop, 0xFF, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(text_count_kernel, dim3(nb), dim3(TX_T), 0, st, d_text, n_scan, cnt, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    unsigned long long breaks = 0;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(&breaks, &d_w->n_breaks, sizeof(breaks), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    *n_lines = (uint64_t) breaks + 1;
    *nb_idx = nb;
    return ECAL_OK;
}

int text_filter_passes(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint64_t n_lines, const ecal_text_options &o,
                       const TextArrays &A, uint8_t *d_events, uint64_t capacity, TextWords *d_w, hipStream_t st) {
    const uint32_t nbl = (uint32_t) ((n_lines + TX_T - 1) / TX_T);
    hipLaunchKernelGGL(text_verdict_kernel, dim3(nbl), dim3(TX_T), 0, st, (const int64_t *) A.stamp, (const uint8_t *) A.status, n_lines, o,
                       A.cls, A.cnt, d_w);
    const int rc = ecal_scan_blocks(ctx, A.cnt, nbl, A.off, st);
    if (rc) return rc;
    hipLaunchKernelGGL(text_write_kernel, dim3(nbl), dim3(TX_T), 0, st, d_text, n_bytes, (const int64_t *) A.stamp, (const double *) A.x,
                       (const double *) A.y, (const uint8_t *) A.pol, (const uint8_t *) A.status, (const uint8_t *) A.cls,
                       (const uint32_t *) A.off, n_lines, o, d_events, capacity, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

// The lines of the kernel's list, parsed on the host and patched into the arrays
int text_host_lines(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint64_t n_lines, uint64_t n_host, const ecal_text_options &o,
                    const TextArrays &A, TextWords *d_w, hipStream_t st) {
    std::vector<uint8_t> text;
    std::vector<uint64_t> line_off;
    std::vector<uint32_t> list;
    std::vector<TextPatch> patch;
    try {
        text.resize(n_bytes);
        line_off.resize(n_lines + 1);
        list.resize(n_host);
        patch.resize(n_host);
    } catch (const std::bad_alloc &) {
        return ECAL_ERR_NOMEM;
    }
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(text.data(), d_text, n_bytes, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(line_off.data(), A.line_off, (n_lines + 1) * 8, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(list.data(), A.host_list, n_host * 4, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    for (uint64_t i = 0; i < n_host; i++) {
        const uint64_t k = list[i];
        if (k >= n_lines) {
            ctx->last_error = "text ingest: the list of host lines is corrupt";
            return ECAL_ERR_HIP;
        }
        const uint64_t b = line_off[k], e = line_off[k + 1] - 1;
        const TextRecord r = text_parse_line_host(text.data() + b, e - b);
        patch[i] = TextPatch{r.stamp, r.x, r.y, (uint32_t) k, r.p, r.status};
    }
    ecal_devbuf d_patch;
    const int rc = ecal_ensure(ctx, d_patch, n_host * sizeof(TextPatch));
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_patch.ptr, patch.data(), n_host * sizeof(TextPatch), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(text_patch_kernel, dim3((uint32_t) ((n_host + TX_T - 1) / TX_T)), dim3(TX_T), 0, st, (const TextPatch *) d_patch.ptr,
                       n_host, o.has_end_stamp, o.end_stamp, A.stamp, A.x, A.y, A.pol, A.status, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (patch and d_patch are this function's)
    return ECAL_OK;
}

// own_events != null: the records go into a buffer allocated here for lines + 1 records (the caller's to hipFree, null when there
// is nothing to free); else into d_events / capacity
int text_ingest(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const ecal_text_options *opt, uint8_t *d_events, uint64_t capacity,
                uint8_t **own_events, ecal_text_info *info, hipStream_t st) {
    ecal_text_options o;
    if (opt) o = *opt; else ecal_text_default_options(&o);
    ecal_text_info I;
    memset(&I, 0, sizeof(I));
    I.time_base = o.has_time_base ? o.time_base : 0;
    if (own_events) *own_events = nullptr;
    if (n_bytes == 0) {
        if (info) *info = I;
        return ECAL_OK;
    }
    const bool trace = ctx->sw.load_trace;
    ecal_load_timer tm("text", trace, st);
    ecal_devbuf idx, lines, words;
    int rc = ecal_ensure(ctx, words, sizeof(TextWords));
    if (rc) return rc;
    TextWords *d_w = words.as<TextWords>();
    tm.mark("start");
    uint64_t n_lines = 0;
    uint32_t nb_idx = 0;
    if ((rc = text_count(ctx, d_text, n_bytes, idx, d_w, &n_lines, &nb_idx, true, st))) return rc;
    I.n_lines = n_lines;
    if (n_lines > 0xFFFFFFFFull) {
        ctx->last_error = "text ingest: more than 2^32-1 lines";
        if (info) *info = I;
        return ECAL_ERR_RANGE;
    }
    const uint32_t nbl = (uint32_t) ((n_lines + TX_T - 1) / TX_T);
    const size_t o_stamp = ((size_t) n_lines + 1) * 8, o_x = o_stamp + (size_t) n_lines * 8, o_y = o_x + (size_t) n_lines * 8,
                 o_list = o_y + (size_t) n_lines * 8, o_cnt = o_list + up8((size_t) n_lines * 4), o_off = o_cnt + up8((size_t) nbl * 4),
                 o_pol = o_off + up8(((size_t) nbl + 1) * 4), o_status = o_pol + up8(n_lines), o_cls = o_status + up8(n_lines),
                 total = o_cls + up8(n_lines);
    if ((rc = ecal_ensure(ctx, lines, total))) return rc;
    uint8_t *base = lines.as<uint8_t>();
    const TextArrays A{(uint64_t *) base,           (int64_t *) (base + o_stamp), (double *) (base + o_x), (double *) (base + o_y),
                       (uint32_t *) (base + o_list), (uint32_t *) (base + o_cnt),  (uint32_t *) (base + o_off), base + o_pol,
                       base + o_status,              base + o_cls};
    if (own_events) {
        capacity = n_lines + 1;
        if ((rc = ecal_ingest_alloc_records(ctx, "text ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    auto fail = [&](int code) { return ecal_ingest_drop_records(own_events, code); };
    uint32_t *idx_cnt = idx.as<uint32_t>(), *idx_off = idx_cnt + nb_idx;
    if ((rc = ecal_scan_blocks(ctx, idx_cnt, nb_idx, idx_off, st))) return fail(rc);
    hipLaunchKernelGGL(text_offsets_kernel, dim3(nb_idx), dim3(TX_T), 0, st, d_text, n_bytes, n_bytes - 1, (const uint32_t *) idx_off, n_lines,
                       A.line_off);
    tm.mark("line index");
    hipLaunchKernelGGL(text_parse_kernel, dim3(nbl), dim3(TX_T), 0, st, d_text, (const uint64_t *) A.line_off, n_lines, o.has_end_stamp,
                       o.end_stamp, A.stamp, A.x, A.y, A.pol, A.status, A.host_list, d_w);
    tm.mark("parse");
    if ((rc = text_filter_passes(ctx, d_text, n_bytes, n_lines, o, A, d_events, capacity, d_w, st))) return fail(rc);
    tm.mark("verdict, scan, write");
    TextWords W;
    auto fetch = [&]() { return ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st); };
    if ((rc = fetch())) return fail(rc);
    I.n_host_lines = W.n_host;
    if (W.n_host) {
        if ((rc = text_host_lines(ctx, d_text, n_bytes, n_lines, W.n_host, o, A, d_w, st))) return fail(rc);
        hipError_t e = hipMemsetAsync(&d_w->first_stop, 0xFF, sizeof(unsigned long long), st);
        if (e == hipSuccess) e = hipMemsetAsync(&d_w->n_events, 0, 4 * sizeof(unsigned long long), st);
        if (e != hipSuccess) {
            ctx->last_error = std::string("text ingest: ") + hipGetErrorString(e);
            return fail(ECAL_ERR_HIP);
        }
        if ((rc = text_filter_passes(ctx, d_text, n_bytes, n_lines, o, A, d_events, capacity, d_w, st))) return fail(rc);
        tm.mark("host lines, filter again");
        if ((rc = fetch())) return fail(rc);
    }
    I.n_blank = W.n_blank;
    if (W.first_bad != TX_NONE) {
        I.first_bad_line = W.first_bad + 1;
        ctx->last_error = "text ingest: malformed line " + std::to_string(I.first_bad_line) +
                          " (four fields: integer stamp, decimal x, decimal y, polarity 0 or 1)";
        if (info) *info = I;
        return fail(ECAL_ERR_INVALID);
    }
    I.n_events = W.n_events;
    I.n_negative = W.n_negative;
    I.n_after_end = W.n_after_end;
    I.n_before_start = W.n_before_start;
    I.time_base = (int64_t) W.base;
    if (info) *info = I;
    if (I.n_events > capacity) {
        ctx->last_error = "text ingest: " + std::to_string(I.n_events) + " records, more than the capacity";
        return fail(ECAL_ERR_RANGE);
    }
    return ECAL_OK;
}

// file -> text in HBM -> records in a device buffer of their own (null for none), the text freed
int text_file_to_events(ecal_ctx *ctx, const char *path, const ecal_text_options *opt, uint8_t **d_events, ecal_text_info *info) {
    *d_events = nullptr;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool trace = ctx->sw.load_trace;
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *d_text = nullptr;
    uint64_t n_bytes = 0;
    int rc = ecal_upload_file(ctx, "text ingest", path, 0, &d_text, &n_bytes);
    if (rc) return rc;
    if (trace)
        fprintf(stderr, "ecal text ingest: %-24s %.3f ms\n", "file read + upload",
                1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    rc = text_ingest(ctx, d_text, n_bytes, opt, nullptr, 0, d_events, info, ctx->stream);
    (void) hipFree(d_text);
    return rc;
}

}  // namespace

int ecal_upload_file(ecal_ctx *ctx, const char *who, const char *path, uint64_t file_offset, uint8_t **d_text_out, uint64_t *n_bytes_out) {
    *d_text_out = nullptr;
    *n_bytes_out = 0;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        ctx->last_error = std::string(who) + ": cannot open " + path;
        return ECAL_ERR_INVALID;
    }
    struct stat sb;
    if (fstat(fd, &sb) != 0) {
        close(fd);
        ctx->last_error = std::string(who) + ": cannot stat " + path;
        return ECAL_ERR_INVALID;
    }
    const uint64_t n = (uint64_t) sb.st_size > file_offset ? (uint64_t) sb.st_size - file_offset : 0;
    constexpr uint64_t CH = 16ull << 20;
    constexpr int NT = 6;
    uint8_t *pin[NT] = {};
    hipEvent_t done[NT] = {};
    uint8_t *d_text = nullptr;
    hipError_t e = hipMalloc((void **) &d_text, (size_t) n + 16);
    const uint64_t n_chunks = (n + CH - 1) / CH;
    const int nt = (int) std::min<uint64_t>(NT, std::max<uint64_t>(n_chunks, 1));
    for (int b = 0; b < nt && e == hipSuccess && n; b++) {
        e = hipHostMalloc((void **) &pin[b], (size_t) std::min<uint64_t>(CH, n), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done[b], hipEventDisableTiming);
    }
    std::atomic<bool> io_error{false};
    if (e == hipSuccess && n) {
        auto reader = [&](int b) {
            if (hipSetDevice(ctx->device) != hipSuccess) io_error = true;
            for (uint64_t k = (uint64_t) b; k < n_chunks && !io_error; k += (uint64_t) nt) {
                const uint64_t b0 = k * CH, want = std::min<uint64_t>(CH, n - b0);
                if (k >= (uint64_t) nt && hipEventSynchronize(done[b]) != hipSuccess) io_error = true;   // the buffer's previous upload
                uint64_t got = 0;
                while (got < want && !io_error) {
                    const ssize_t rd = pread(fd, pin[b] + got, want - got, (off_t) (file_offset + b0 + got));
                    if (rd <= 0) io_error = true;
                    else got += (uint64_t) rd;
                }
                if (io_error) break;
                if (hipMemcpyAsync(d_text + b0, pin[b], want, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                    hipEventRecord(done[b], ctx->stream) != hipSuccess)
                    io_error = true;
            }
        };
        std::vector<std::thread> th;
        for (int b = 1; b < nt; b++) th.emplace_back(reader, b);
        reader(0);
        for (auto &t : th) t.join();
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) io_error = true;
    }
    for (int b = 0; b < NT; b++) {
        if (done[b]) (void) hipEventDestroy(done[b]);
        if (pin[b]) (void) hipHostFree(pin[b]);
    }
    close(fd);
    if (e != hipSuccess || io_error) {
        ctx->last_error = e != hipSuccess ? std::string(who) + ": " + hipGetErrorString(e)
                                          : std::string(who) + ": read or copy failed for " + path;
        if (d_text) (void) hipFree(d_text);
        return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
    }
    *d_text_out = d_text;
    *n_bytes_out = n;
    return ECAL_OK;
}

int ecal_write_records_file(ecal_ctx *ctx, const char *who, const uint8_t *d_events, uint64_t n_events, const char *bin_path,
                            const std::string *prefix) {
    const int fd = open(bin_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) {
        ctx->last_error = std::string(who) + ": cannot write " + bin_path;
        return ECAL_ERR_INVALID;
    }
    for (size_t put = 0; prefix && put < prefix->size();) {
        const ssize_t wr = write(fd, prefix->data() + put, prefix->size() - put);
        if (wr <= 0) {
            close(fd);
            ctx->last_error = std::string(who) + ": write failed for " + bin_path;
            return ECAL_ERR_INVALID;
        }
        put += (size_t) wr;
    }
    // the records come down through pinned staging, a chunk at a time
    const uint64_t bytes = n_events * 25;
    const size_t CH = 32u << 20;
    unsigned char *stage = bytes ? ecal_fetch_pinned(ctx, (size_t) std::min<uint64_t>(CH, bytes)) : nullptr;
    std::vector<unsigned char> pageable;
    if (bytes && !stage) {
        pageable.resize((size_t) std::min<uint64_t>(CH, bytes));
        stage = pageable.data();
    }
    int rc = ECAL_OK;
    for (uint64_t at = 0; at < bytes && rc == ECAL_OK; at += CH) {
        const size_t n = (size_t) std::min<uint64_t>(CH, bytes - at);
        if (hipMemcpy(stage, d_events + at, n, hipMemcpyDeviceToHost) != hipSuccess) {
            ctx->last_error = std::string(who) + ": download failed";
            rc = ECAL_ERR_HIP;
        }
        for (size_t put = 0; put < n && rc == ECAL_OK;) {
            const ssize_t wr = write(fd, stage + put, n - put);
            if (wr <= 0) {
                ctx->last_error = std::string(who) + ": write failed for " + bin_path;
                rc = ECAL_ERR_INVALID;
            } else {
                put += (size_t) wr;
            }
        }
    }
    if (close(fd) != 0 && rc == ECAL_OK) {
        ctx->last_error = std::string(who) + ": write failed for " + bin_path;
        rc = ECAL_ERR_INVALID;
    }
    return rc;
}

extern "C" int ecal_text_count_lines_dev(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint64_t *n_lines, void *stream) {
    if (!ctx || !n_lines) return ECAL_ERR_INVALID;
    int rc = ecal_ingest_check_buffer(ctx, "text ingest", d_text, n_bytes, 16, "text");
    if (rc) return rc;
    *n_lines = 0;
    if (!n_bytes) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ecal_devbuf idx, words;
    if ((rc = ecal_ensure(ctx, words, sizeof(TextWords)))) return rc;
    uint64_t n = 0;
    uint32_t nb = 0;
    if ((rc = text_count(ctx, d_text, n_bytes, idx, words.as<TextWords>(), &n, &nb, false, (hipStream_t) stream))) return rc;
    *n_lines = n;
    return ECAL_OK;
}

extern "C" int ecal_events_from_text_dev(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const ecal_text_options *opt,
                                         uint8_t *d_events, uint64_t capacity, ecal_text_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_text");
    if (!ctx) return ECAL_ERR_INVALID;
    const int rc = ecal_ingest_check_buffer(ctx, "text ingest", d_text, n_bytes, 16, "text");
    if (rc) return rc;
    if (capacity && !d_events) {
        ctx->last_error = "text ingest: null record buffer";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return text_ingest(ctx, d_text, n_bytes, opt, d_events, capacity, nullptr, info, (hipStream_t) stream);
}

extern "C" int ecal_stream_create_from_text_file(ecal_ctx *ctx, const char *path, const ecal_text_options *opt, ecal_stream **out,
                                                 ecal_text_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_text_info I;
    memset(&I, 0, sizeof(I));
    int rc = text_file_to_events(ctx, path, opt, &d_events, &I);
    if (info) *info = I;
    if (rc) return rc;
    if (I.n_events > 0xFFFFFFFFull) {
        if (d_events) (void) hipFree(d_events);
        ctx->last_error = "more than 2^32-1 events in one stream";
        return ECAL_ERR_RANGE;
    }
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_text_file", d_events, I.n_events, out);
}

extern "C" int ecal_text_to_bin_file(ecal_ctx *ctx, const char *txt_path, const char *bin_path, const ecal_text_options *opt,
                                     ecal_text_info *info) {
    if (!ctx || !txt_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_text_info I;
    memset(&I, 0, sizeof(I));
    const int rc = text_file_to_events(ctx, txt_path, opt, &d_events, &I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_text_to_bin_file", d_events, I.n_events, bin_path);
}
