// Pixel activity and the hot-pixel filter (include/ecal.h, "pixel activity / hot pixels"): how many events every sensor pixel fired,
// the rule that calls a pixel hot, and the stream without the events of the masked pixels.  What decides — the pixel of a record, the
// rule, keep or remove — is pixel_activity.hpp's (shared with the CPU test); design/17_hot_pixels.md has the reasoning.
//
// Blocks of PA_BLOCK consecutive events per workgroup over the packed 25-byte records, and NO waiting between workgroups:
//   pixel_activity_kernel      one pass; one u32 atomic per on-grid event into counts[2][H][W] (the access shape of the board image's
//                              atomics), the totals reduced in the block: one atomic per block and counter.  Integer atomics only: the
//                              map does not depend on the order of arrival.
//   activity_verdict_kernel    one keep / remove byte per event from the u8 mask, the kept events per block, the totals
//   ecal_scan_blocks           the blocks' first kept index (the association's)
//   activity_write_kernel      compact_write_block (stream_compact.hpp) with the kept events' own 25 bytes
// The scan and the writing pass are ecal_compact_copy_by_verdict (ecal_ctx.hpp): the noise filter (ecal_noise.hip) ends in them too.
// This file also holds the host steps every compacting stage shares (ecal_ctx.hpp, "what the compacting stages share").
// Bytes per event: 25 read + 4 atomic in the activity pass; 17 read (x, y, the mask byte) + 1 written in the verdict pass; 1 read in
// the writing pass, and per KEPT event 25 read + 25 written.
// Nothing behind n_events * 25 bytes of the input is loaded and nothing behind the kept records is stored: any caller tensor will do.
#include <hip/hip_runtime.h>
#include <vector>
#include "ecal_ctx.hpp"
#include "pixel_activity.hpp"
#include "stream_compact.hpp"

namespace ecal {

using namespace ecal_activity;

static_assert(ECAL_ERR_INVALID == PA_INVALID && ECAL_OK == PA_OK, "status codes");

constexpr int PA_T = SC_T;
constexpr uint32_t PA_BLOCK = SC_BLOCK;

// counts: [2][height][width], zero before the launch; totals (may be null): n_events, n_on_grid, n_off_grid, zero before the launch
__global__ __launch_bounds__(PA_T) void pixel_activity_kernel(const uint8_t *__restrict__ rec, uint64_t n_events, uint32_t width,
                                                              uint32_t height, uint32_t *__restrict__ counts,
                                                              unsigned long long *__restrict__ totals) {
    __shared__ uint32_t s_red[PA_T / 64];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * PA_BLOCK;
    const uint32_t count = stream_block_count(n_events, base);
    const uint8_t *const blk = rec + base * PA_RECORD_BYTES;
    const size_t plane = (size_t) width * height;
    uint32_t on = 0;
    for (uint32_t k = (uint32_t) tid; k < count; k += PA_T) {
        const uint8_t *r = blk + (size_t) k * PA_RECORD_BYTES;
        const uint32_t p = pa_record_pixel(r, width, height);   // (< plane, or PA_OFF_GRID)
        if (p != PA_OFF_GRID) {
            on++;
            atomicAdd(&counts[pa_record_plane(r) * plane + p], 1u);
        }
    }
    if (!totals) return;
    on = block_sum<PA_T>(on, s_red);
    if (tid == 0) atomicAdd(&totals[0], (unsigned long long) count);
    if (tid == 1 && on) atomicAdd(&totals[1], (unsigned long long) on);
    if (tid == 2 && count - on) atomicAdd(&totals[2], (unsigned long long) (count - on));
}

// verdict: one byte per event (1 keep, 0 remove); block_cnt: the kept events of every block; totals (may be null): n_events,
// n_off_grid, n_removed, n_kept, zero before the launch
__global__ __launch_bounds__(PA_T) void activity_verdict_kernel(const uint8_t *__restrict__ rec, uint64_t n_events,
                                                                const uint8_t *__restrict__ mask, uint32_t width, uint32_t height,
                                                                uint8_t *__restrict__ verdict, uint32_t *__restrict__ block_cnt,
                                                                unsigned long long *__restrict__ totals) {
    __shared__ uint32_t s_red[2][PA_T / 64];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * PA_BLOCK;
    const uint32_t count = stream_block_count(n_events, base);
    const uint8_t *const blk = rec + base * PA_RECORD_BYTES;
    uint32_t keep = 0, off = 0;
    for (uint32_t k = (uint32_t) tid; k < count; k += PA_T) {
        bool og;
        const uint8_t v = pa_record_keep(blk + (size_t) k * PA_RECORD_BYTES, mask, width, height, &og);
        verdict[base + k] = v;
        keep += v;
        off += og ? 1u : 0u;
    }
    keep = block_sum<PA_T>(keep, s_red[0]);
    off = block_sum<PA_T>(off, s_red[1]);
    if (tid == 0) block_cnt[blockIdx.x] = keep;
    if (!totals) return;
    if (tid == 0) atomicAdd(&totals[0], (unsigned long long) count);
    if (tid == 1 && off) atomicAdd(&totals[1], (unsigned long long) off);
    if (tid == 2 && count - keep) atomicAdd(&totals[2], (unsigned long long) (count - keep));
    if (tid == 3 && keep) atomicAdd(&totals[3], (unsigned long long) keep);
}

// verdict: rounded up to whole blocks (the bytes behind n_events are read and masked, never written); out: room for the kept records
__global__ __launch_bounds__(PA_T) void activity_write_kernel(const uint8_t *__restrict__ rec, uint64_t n_events,
                                                              const uint8_t *__restrict__ verdict, const uint32_t *__restrict__ block_off,
                                                              uint8_t *__restrict__ out) {
    compact_write_block(rec, n_events, verdict, block_off, out, [](const uint8_t *r, uint8_t *d) {
        uint64_t a0, a1, a2;
        __builtin_memcpy(&a0, r, 8);
        __builtin_memcpy(&a1, r + 8, 8);
        __builtin_memcpy(&a2, r + 16, 8);
        const uint8_t a3 = r[24];
        __builtin_memcpy(d, &a0, 8);
        __builtin_memcpy(d + 8, &a1, 8);
        __builtin_memcpy(d + 16, &a2, 8);
        d[24] = a3;
    });
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_activity_totals) == 24 && sizeof(ecal_filter_totals) == 32, "the totals have no padding");
static_assert(sizeof(ecal_hot_pixel_options) == sizeof(HotOptions) && sizeof(ecal_hot_pixel_info) == sizeof(HotInfo) &&
                  sizeof(ecal_hot_pixel_options) == 24 && sizeof(ecal_hot_pixel_info) == 56,
              "the options and the info are the shared header's");

extern "C" void ecal_hot_pixel_default_options(ecal_hot_pixel_options *opt) {
    if (!opt) return;
    opt->width = PA_DEFAULT_WIDTH;
    opt->height = PA_DEFAULT_HEIGHT;
    opt->quantile_permille = PA_DEFAULT_QUANTILE_PERMILLE;
    opt->min_count = PA_DEFAULT_MIN_COUNT;
    opt->factor = PA_DEFAULT_FACTOR;
}

static HotOptions hot_options(const ecal_hot_pixel_options *opt) {
    ecal_hot_pixel_options o;
    if (opt) o = *opt; else ecal_hot_pixel_default_options(&o);
    return HotOptions{o.width, o.height, o.quantile_permille, o.min_count, o.factor};
}

static void hot_info_out(ecal_hot_pixel_info *info, const HotInfo &I) {
    if (!info) return;
    info->n_events = I.n_events;
    info->n_off_grid = I.n_off_grid;
    info->n_removed = I.n_removed;
    info->n_kept = I.n_kept;
    info->n_active_pixels = I.n_active_pixels;
    info->n_hot_pixels = I.n_hot_pixels;
    info->n_masked_pixels = I.n_masked_pixels;
    info->quantile_count = I.quantile_count;
    info->max_count = I.max_count;
    info->max_kept_count = I.max_kept_count;
}

extern "C" int ecal_hot_pixel_mask(const uint32_t *counts, const ecal_hot_pixel_options *opt, const uint8_t *extra_mask, uint8_t *mask,
                                   ecal_hot_pixel_info *info) {
    HotInfo I;
    memset(&I, 0, sizeof(I));
    hot_info_out(info, I);
    const int rc = pa_hot_pixel_mask(counts, hot_options(opt), extra_mask, mask, &I);
    if (rc) return rc;
    hot_info_out(info, I);
    return ECAL_OK;
}

// ---- what the compacting stages share (ecal_ctx.hpp) ----
static_assert(ECAL_STREAM_BLOCK == SC_BLOCK, "the host's blocks are the kernels'");

int ecal_verdict_tables_ensure(ecal_ctx *ctx, ecal_devbuf &scratch, uint64_t n_events, ecal_verdict_tables *V) {
    const uint32_t nb = ecal_stream_blocks(n_events);
    const int rc = ecal_ensure(ctx, scratch, ecal_verdict_tables_bytes(nb));
    if (rc) return rc;
    *V = ecal_verdict_tables_at(scratch.as<uint8_t>(), nb);
    return ECAL_OK;
}

int ecal_events_range_check(ecal_ctx *ctx, const char *who, uint64_t n_events) {
    if (n_events > 0xFFFFFFFFull) {
        ctx->last_error = std::string(who) + ": more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

int ecal_compact_begin(ecal_ctx *ctx, const char *who, const uint8_t *d_events, uint64_t n_events, const uint8_t *d_out, uint32_t *d_count,
                       void *d_totals, size_t totals_bytes, hipStream_t st) {
    const size_t bytes = (size_t) n_events * PA_RECORD_BYTES;
    if (n_events && d_out && d_events < d_out + bytes && d_out < d_events + bytes) {
        ctx->last_error = std::string(who) + ": the output overlaps the events";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_count, 0, sizeof(uint32_t), st));
    if (d_totals) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_totals, 0, totals_bytes, st));
    return ECAL_OK;
}

int ecal_compact_copy_by_verdict(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_verdict_tables &V, uint8_t *d_out,
                                 uint32_t *d_count, ecal_load_timer &tm, hipStream_t st) {
    return ecal_compact_by_verdict(ctx, V, d_count, &tm, st, [&]() {
        hipLaunchKernelGGL(activity_write_kernel, dim3(V.nb), dim3(PA_T), 0, st, d_events, n_events, (const uint8_t *) V.verdict,
                           (const uint32_t *) V.off, d_out);
    });
}

int ecal_stream_compacted(ecal_ctx *ctx, const char *who, const ecal_stream *in, void *d_results, void *totals, size_t totals_bytes,
                          const ecal_stream_dev_fn &run_dev, const ecal_stream_disagree_fn &disagree, ecal_stream **out) {
    const uint64_t n = ecal_stream_size(in);
    hipStream_t st = ctx->stream;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_results) + totals_bytes);
    uint8_t *d_out = nullptr;
    int rc = ecal_ingest_alloc_records(ctx, who, n, &d_out);
    if (rc) {
        (void) hipStreamSynchronize(st);   // (a caller's upload may still read host memory that goes out of scope with this return)
        return rc;
    }
    uint32_t kept = 0;
    auto run = [&]() -> int {
        const int frc = run_dev(d_out, d_count, d_results, st);
        if (frc) return frc;
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(totals, d_results, totals_bytes, hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(&kept, d_count, sizeof(kept), hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
        return ECAL_OK;
    };
    rc = run();
    if (rc) {
        (void) hipStreamSynchronize(st);
        return ecal_ingest_drop_records(&d_out, rc);
    }
    if (const char *bad = disagree(kept, n)) {
        ctx->last_error = std::string(who) + ": " + bad;
        return ecal_ingest_drop_records(&d_out, ECAL_ERR_HIP);
    }
    return ecal_stream_from_events(ctx, who, d_out, kept, out);
}

static int activity_check(ecal_ctx *ctx, const char *who, uint64_t n_events, uint32_t width, uint32_t height) {
    if (!pa_size_ok(width, height)) {
        ctx->last_error = std::string(who) + ": width and height from 1 to 4096";
        return ECAL_ERR_INVALID;
    }
    return ecal_events_range_check(ctx, who, n_events);
}

extern "C" int ecal_pixel_activity_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, uint32_t width, uint32_t height,
                                       uint32_t *d_counts, ecal_activity_totals *d_totals, void *stream) {
    const ecal_range range__(ctx, "ecal_pixel_activity");
    if (!ctx) return ECAL_ERR_INVALID;
    if (!d_counts || (n_events && !d_events)) {
        ctx->last_error = "ecal_pixel_activity: null pointer (counts or events)";
        return ECAL_ERR_INVALID;
    }
    const int rc = activity_check(ctx, "ecal_pixel_activity", n_events, width, height);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, 2 * (size_t) width * height * sizeof(uint32_t), st));
    if (d_totals) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_totals, 0, sizeof(ecal_activity_totals), st));
    if (!n_events) return ECAL_OK;
    const uint32_t nb = (uint32_t) ((n_events + PA_BLOCK - 1) / PA_BLOCK);
    ecal_load_timer tm("pixel activity", ctx->sw.load_trace, st);
    tm.mark("start");
    hipLaunchKernelGGL(pixel_activity_kernel, dim3(nb), dim3(PA_T), 0, st, d_events, n_events, width, height, d_counts,
                       (unsigned long long *) d_totals);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark("count");
    if (tm.on) ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (ECAL_TRACE=load alone: the timer reads its events when it goes out of scope)
    return ECAL_OK;
}

extern "C" int ecal_filter_events_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const uint8_t *d_mask, uint32_t width,
                                      uint32_t height, uint8_t *d_out, uint32_t *d_count, ecal_filter_totals *d_totals, void *stream) {
    const ecal_range range__(ctx, "ecal_filter_events");
    if (!ctx) return ECAL_ERR_INVALID;
    if (!d_mask || !d_count || (n_events && (!d_events || !d_out))) {
        ctx->last_error = "ecal_filter_events: null pointer (mask, count, events or output)";
        return ECAL_ERR_INVALID;
    }
    int rc = activity_check(ctx, "ecal_filter_events", n_events, width, height);
    if (rc) return rc;
    hipStream_t st = (hipStream_t) stream;
    if ((rc = ecal_compact_begin(ctx, "ecal_filter_events", d_events, n_events, d_out, d_count, d_totals, sizeof(ecal_filter_totals), st))) return rc;
    if (!n_events) return ECAL_OK;
    ecal_verdict_tables V;
    if ((rc = ecal_verdict_tables_ensure(ctx, ctx->activity_scratch, n_events, &V))) return rc;
    ecal_load_timer tm("hot pixel filter", ctx->sw.load_trace, st);
    tm.mark("start");
    hipLaunchKernelGGL(activity_verdict_kernel, dim3(V.nb), dim3(PA_T), 0, st, d_events, n_events, d_mask, width, height, V.verdict, V.cnt,
                       (unsigned long long *) d_totals);
    tm.mark("verdict");
    rc = ecal_compact_copy_by_verdict(ctx, d_events, n_events, V, d_out, d_count, tm, st);
    if (rc) return rc;
    if (tm.on) ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (ECAL_TRACE=load alone: the timer reads its events when it goes out of scope)
    return ECAL_OK;
}

extern "C" int ecal_stream_remove_hot_pixels(ecal_ctx *ctx, const ecal_stream *in, const ecal_hot_pixel_options *opt, const uint8_t *extra_mask,
                                             ecal_stream **out, uint8_t *mask_out, uint32_t *counts_out, ecal_hot_pixel_info *info) {
    if (!ctx || !in || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    HotInfo I;
    memset(&I, 0, sizeof(I));
    hot_info_out(info, I);
    const HotOptions o = hot_options(opt);
    if (!pa_options_ok(o)) {
        ctx->last_error = "ecal_stream_remove_hot_pixels: width and height from 1 to 4096, quantile_permille <= 1000, a finite factor >= 0";
        return ECAL_ERR_INVALID;
    }
    const uint64_t n = ecal_stream_size(in);
    const uint8_t *d_in = ecal_stream_data(in);
    const size_t plane = (size_t) o.width * o.height;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // counts [2][plane] u32 | filter totals | count | mask [plane]
    const size_t o_tot = 2 * plane * 4, o_cnt = o_tot + sizeof(ecal_filter_totals), o_mask = o_cnt + 8, total = o_mask + plane;
    int rc = ecal_ensure(ctx, ctx->activity_maps, total);
    if (rc) return rc;
    uint8_t *base = ctx->activity_maps.as<uint8_t>();
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(base);   // (the count stands behind the totals: ecal_stream_compacted's results)
    ecal_filter_totals *d_tot = reinterpret_cast<ecal_filter_totals *>(base + o_tot);
    uint8_t *d_mask = base + o_mask;
    // 1. the count map, and the small trip to the host for the rule (one-off ingest work)
    rc = ecal_pixel_activity_dev(ctx, d_in, n, o.width, o.height, d_counts, nullptr, st);
    if (rc) return rc;
    std::vector<uint32_t> counts_own;
    uint32_t *counts = counts_out;
    if (!counts) {
        counts_own.resize(2 * plane);
        counts = counts_own.data();
    }
    std::vector<uint8_t> mask_own;
    uint8_t *mask = mask_out;
    if (!mask) {
        mask_own.resize(plane);
        mask = mask_own.data();
    }
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, 2 * plane * 4, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    rc = pa_hot_pixel_mask(counts, o, extra_mask, mask, &I);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_mask, mask, plane, hipMemcpyHostToDevice, st));
    // 2. the filter into records of the new stream's own (every event may stay); the helper synchronises the stream before it
    // returns, whatever happens: the mask's upload reads host memory that goes out of scope here
    ecal_filter_totals T;
    return ecal_stream_compacted(
        ctx, "ecal_stream_remove_hot_pixels", in, d_tot, &T, sizeof(T),
        [&](uint8_t *d_out, uint32_t *d_cnt, void *d_totals, hipStream_t s) {
            return ecal_filter_events_dev(ctx, d_in, n, d_mask, o.width, o.height, d_out, d_cnt, (ecal_filter_totals *) d_totals, s);
        },
        [&](uint32_t kept, uint64_t n_in) -> const char * {
            I.n_events = T.n_events;
            I.n_off_grid = T.n_off_grid;
            I.n_removed = T.n_removed;
            I.n_kept = T.n_kept;
            hot_info_out(info, I);
            return T.n_kept != kept || T.n_removed + T.n_kept != n_in ? "the filter's counters disagree" : nullptr;
        },
        out);
}
