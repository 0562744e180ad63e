// Undistortion with the solved camera (include/ecal.h, "undistortion"): the stream whose events stand where the ideal pinhole camera
// would have seen them, and the reference's undistorted event frames.  What decides — the rule for a point, the rounding to a canvas
// pixel, kept / invalid / outside — is undistort_point.hpp's (shared with the host entry point and the CPU test);
// design/20_undistort.md has the reasoning.
//
// The stream form is the three launches both filters have, blocks of PA_BLOCK_EVENTS events per workgroup, NO waiting between
// workgroups:
//   undistort_verdict_kernel   reads the 16 coordinate bytes of each record: a keep byte per event, the kept events per block, the totals
//   ecal_scan_blocks           the blocks' first kept index (the association's)
//   undistort_write_kernel     compact_write_block (stream_compact.hpp), the writing pass of the filters, with x and y RECOMPUTED
//                              where a record is staged in LDS (about 25 f64 operations: cheaper than carrying 16 more bytes an event
//                              through HBM between the passes)
// Bytes per event: 16 read + 1 written in the verdict pass; 1 read in the writing pass, and per KEPT event 25 read + 25 written.
// No per-pixel lookup table: the rule must hold for off-grid and sub-pixel inputs too, and the arithmetic is cheaper than the gather.
//
// The frames: one workgroup per window.  Two presence bits per canvas pixel (positive, negative), set with atomic OR — integer, so the
// picture does not depend on the order of arrival — in LDS when the canvas fits (415 x 312: 32 372 bytes), else in zeroed context
// scratch; then the bits expanded to RGB with aligned 4-byte stores.
// Nothing behind n_events * 25 bytes of the input is loaded and nothing behind the kept records is stored: any caller tensor will do.
#include <hip/hip_runtime.h>
#include <vector>
#include "ecal_ctx.hpp"
#include "stream_compact.hpp"
#include "undistort_point.hpp"

namespace ecal {

using namespace ecal_undistort;

constexpr int UD_T = SC_T;
constexpr uint32_t UD_BLOCK = SC_BLOCK;
static_assert(UD_RECORD_BYTES == SC_RECORD, "one record layout");

constexpr uint32_t UF_T = 256;
constexpr uint32_t UF_LDS_WORDS = 8192;            // 32 KB of presence bits: canvases up to 131 072 pixels (the reference's 415 x 312 = 129 480)
constexpr uint32_t UF_PIXELS_PER_WORD = 16;

// uv [n][2], flag [n]: the rule per record (0, 0 and flag 1 where invalid)
__global__ __launch_bounds__(UD_T) void undistort_points_kernel(const Camera cam, const uint8_t *__restrict__ rec, uint32_t n_events,
                                                                double *__restrict__ uv, uint8_t *__restrict__ flag) {
    const uint64_t i = (uint64_t) blockIdx.x * UD_T + threadIdx.x;
    if (i >= (uint64_t) n_events) return;
    const uint8_t *r = rec + (size_t) i * UD_RECORD_BYTES;
    double up = 0.0, vp = 0.0;
    const bool ok = ud_point(cam, ud_load_f64(r + 8), ud_load_f64(r + 16), &up, &vp);
    uv[2 * i] = ok ? up : 0.0;
    uv[2 * i + 1] = ok ? vp : 0.0;
    flag[i] = ok ? 0 : 1;
}

// verdict: one byte per event (1 keep, 0 remove); block_cnt: the kept events of every block; totals (may be null): n_events,
// n_invalid, n_outside, n_kept, zero before the launch
__global__ __launch_bounds__(UD_T) void undistort_verdict_kernel(const Camera cam, const Options opt, const uint8_t *__restrict__ rec,
                                                                 uint64_t n_events, uint8_t *__restrict__ verdict,
                                                                 uint32_t *__restrict__ block_cnt, unsigned long long *__restrict__ totals) {
    __shared__ uint32_t s_red[3][UD_T / 64];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * UD_BLOCK;
    const uint32_t count = stream_block_count(n_events, base);
    const uint8_t *const blk = rec + base * UD_RECORD_BYTES;
    uint32_t keep = 0, inv = 0, outside = 0;
    for (uint32_t k = (uint32_t) tid; k < count; k += UD_T) {
        const uint8_t *r = blk + (size_t) k * UD_RECORD_BYTES;
        double ox, oy;
        const uint32_t what = ud_event(cam, opt, ud_load_f64(r + 8), ud_load_f64(r + 16), &ox, &oy);
        verdict[base + k] = (uint8_t) (what == UD_KEPT ? 1u : 0u);
        keep += what == UD_KEPT ? 1u : 0u;
        inv += what == UD_INVALID ? 1u : 0u;
        outside += what == UD_OUTSIDE ? 1u : 0u;
    }
    keep = block_sum<UD_T>(keep, s_red[0]);
    inv = block_sum<UD_T>(inv, s_red[1]);
    outside = block_sum<UD_T>(outside, s_red[2]);
    if (tid == 0) block_cnt[blockIdx.x] = keep;
    if (!totals) return;
    if (tid == 0) atomicAdd(&totals[0], (unsigned long long) count);
    if (tid == 1 && inv) atomicAdd(&totals[1], (unsigned long long) inv);
    if (tid == 2 && outside) atomicAdd(&totals[2], (unsigned long long) outside);
    if (tid == 3 && keep) atomicAdd(&totals[3], (unsigned long long) keep);
}

// verdict: rounded up to whole blocks (the bytes behind n_events are read and masked, never written); out: room for the kept records
__global__ __launch_bounds__(UD_T) void undistort_write_kernel(const Camera cam, const Options opt, const uint8_t *__restrict__ rec,
                                                               uint64_t n_events, const uint8_t *__restrict__ verdict,
                                                               const uint32_t *__restrict__ block_off, uint8_t *__restrict__ out) {
    // x and y are replaced on the way into LDS
    compact_write_block(rec, n_events, verdict, block_off, out, [&](const uint8_t *r, uint8_t *d) {
        uint64_t a0;
        double x, y, ox = 0.0, oy = 0.0;
        __builtin_memcpy(&a0, r, 8);
        __builtin_memcpy(&x, r + 8, 8);
        __builtin_memcpy(&y, r + 16, 8);
        const uint8_t a3 = r[24];
        (void) ud_event(cam, opt, x, y, &ox, &oy);   // (UD_KEPT: the verdict pass saw the same bytes)
        __builtin_memcpy(d, &a0, 8);
        __builtin_memcpy(d + 8, &ox, 8);
        __builtin_memcpy(d + 16, &oy, 8);
        d[24] = a3;
    });
}

// Window s = blockIdx.x.  bits: the window's n_words presence words (LDS: the kernel's own, zeroed here; else g_bits + s * n_words,
// zero before the launch).  Pixel p = Y * out_width + X: bit 2 * (p % 16) of word p / 16 positive, the bit above it negative.
template <bool LDS>
__global__ __launch_bounds__(UF_T) void undistorted_frames_kernel(const Camera cam, const Options opt, const double *__restrict__ xy,
                                                                  const uint32_t *__restrict__ xy16, const uint32_t *__restrict__ seg_fmt,
                                                                  const uint32_t *__restrict__ seg_off, const uint32_t *__restrict__ seg_cnt,
                                                                  uint32_t n_words, uint32_t *__restrict__ g_bits, uint8_t *__restrict__ rgb,
                                                                  FrameTotals *__restrict__ frame_totals) {
    __shared__ uint32_t s_bits[LDS ? UF_LDS_WORDS : 1];
    __shared__ uint32_t s_red[4][UF_T / 64];
    const uint32_t tid = threadIdx.x, s = blockIdx.x;
    uint32_t *const bits = LDS ? s_bits : g_bits + (size_t) s * n_words;
    if (LDS) {
        for (uint32_t j = tid; j < n_words; j += UF_T) s_bits[j] = 0u;
        __syncthreads();
    }
    uint32_t painted[2] = {0, 0}, inv = 0, outside = 0;
#pragma unroll
    for (uint32_t pol = 0; pol < 2; pol++) {   // segment 2s: the positive points, 2s + 1: the negative ones
        const uint32_t seg = 2u * s + pol, off = seg_off[seg], cnt = seg_cnt[seg];
        const bool packed = xy16 && seg_fmt && (seg_fmt[seg] & 1u);
        for (uint32_t i = tid; i < cnt; i += UF_T) {
            double u, v;
            if (packed) {
                const uint32_t wv = xy16[off + i];
                u = (double) (int16_t) (wv & 0xFFFFu);
                v = (double) (int16_t) (wv >> 16);
            } else {
                u = xy[2 * (size_t) (off + i)];
                v = xy[2 * (size_t) (off + i) + 1];
            }
            double X, Y;
            const uint32_t what = ud_event(cam, opt, u, v, &X, &Y);
            if (what == UD_KEPT) {
                const uint32_t p = (uint32_t) Y * opt.out_width + (uint32_t) X;   // (< out_width * out_height <= 16 * n_words)
                atomicOr(&bits[p / UF_PIXELS_PER_WORD], 1u << (2u * (p % UF_PIXELS_PER_WORD) + pol));
                painted[pol]++;
            } else if (what == UD_INVALID) {
                inv++;
            } else {
                outside++;
            }
        }
    }
    if (frame_totals) {
        const uint32_t a = block_sum<UF_T>(painted[0], s_red[0]), b = block_sum<UF_T>(painted[1], s_red[1]);
        const uint32_t c = block_sum<UF_T>(inv, s_red[2]), d = block_sum<UF_T>(outside, s_red[3]);
        if (tid == 0) frame_totals[s] = FrameTotals{a, b, c, d};
    }
    __syncthreads();   // (the atomics of this workgroup: LDS, or device memory no other workgroup touches)
    // expansion: byte j of the window's picture is channel j % 3 of pixel j / 3; bytes up to the first 4-byte boundary, whole words,
    // the bytes behind them
    const uint32_t nbytes = opt.out_width * opt.out_height * 3u;   // <= 8192 * 8192 * 3 < 2^32
    uint8_t *const dst = rgb + (size_t) s * nbytes;
    auto byte_at = [&](uint32_t j) -> uint32_t {
        const uint32_t p = j / 3u, ch = j - 3u * p;
        const uint32_t wv = LDS ? bits[p / UF_PIXELS_PER_WORD] : __hip_atomic_load(&bits[p / UF_PIXELS_PER_WORD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t two = (wv >> (2u * (p % UF_PIXELS_PER_WORD))) & 3u;   // bit 0 positive, bit 1 negative
        const bool on = ch == 0u ? two == 1u : (ch == 1u ? (two & 2u) != 0u : false);
        return on ? 255u : 0u;
    };
    uint32_t head = (uint32_t) ((4u - ((uintptr_t) dst & 3u)) & 3u);
    head = head < nbytes ? head : nbytes;
    const uint32_t nw = (nbytes - head) / 4u;
    if (tid < head) dst[tid] = (uint8_t) byte_at(tid);
    for (uint32_t j = tid; j < nw; j += UF_T) {
        const uint32_t at = head + 4u * j;
        const uint32_t v = byte_at(at) | (byte_at(at + 1u) << 8) | (byte_at(at + 2u) << 16) | (byte_at(at + 3u) << 24);
        *reinterpret_cast<uint32_t *>(dst + at) = v;
    }
    const uint32_t tail0 = head + 4u * nw;
    if (tail0 + tid < nbytes) dst[tail0 + tid] = (uint8_t) byte_at(tail0 + tid);   // (fewer than 4 bytes)
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_undistort_camera) == sizeof(Camera) && sizeof(ecal_undistort_camera) == 112, "the camera is the shared header's, no padding");
static_assert(sizeof(ecal_undistort_options) == sizeof(Options) && sizeof(ecal_undistort_options) == 32, "the options are the shared header's");
static_assert(sizeof(ecal_undistort_totals) == sizeof(Totals) && sizeof(ecal_undistort_frame_totals) == sizeof(FrameTotals), "the totals are the shared header's");
static_assert(ECAL_CAMERA_RADIAL == UD_RADIAL && ECAL_CAMERA_FISHEYE == UD_FISHEYE && ECAL_UNDISTORT_PIXEL == UD_PIXEL, "the shared header's constants");

extern "C" void ecal_undistort_camera_from_params(int model, const double *params9, ecal_undistort_camera *cam) {
    if (!cam) return;
    memset(cam, 0, sizeof(*cam));
    cam->model = model;
    if (!params9) return;
    for (int i = 0; i < 9; i++) cam->intr[i] = params9[i];
    for (int i = 0; i < 4; i++) cam->out_k[i] = params9[i];
}

extern "C" void ecal_undistort_reference_canvas(uint32_t width, uint32_t height, ecal_undistort_options *opt) {
    if (!opt) return;
    const Options o = ud_reference_canvas(width, height);
    memcpy(opt, &o, sizeof(o));
}

static Camera ud_camera(const ecal_undistort_camera *cam) {
    Camera c;
    memcpy(&c, cam, sizeof(c));
    return c;
}

static Options ud_options(const ecal_undistort_options *opt) {
    Options o;
    memset(&o, 0, sizeof(o));   // SUBPIXEL
    if (opt) memcpy(&o, opt, sizeof(o));
    return o;
}

extern "C" const char *ecal_undistort_camera_error(const ecal_undistort_camera *cam) {
    if (!cam) return "null camera";
    return ud_camera_error(ud_camera(cam));
}

extern "C" const char *ecal_undistort_options_error(const ecal_undistort_options *opt) { return ud_options_error(ud_options(opt)); }

extern "C" double ecal_undistort_round_half_away(double a) { return ud_round_half_away(a); }

extern "C" int ecal_undistort_points_host(const ecal_undistort_camera *cam, const double *uv, uint64_t n, double *out, uint8_t *flag) {
    if (ecal_undistort_camera_error(cam) || (n && (!uv || !out || !flag))) return ECAL_ERR_INVALID;
    const Camera c = ud_camera(cam);
    for (uint64_t i = 0; i < n; i++) {
        double up = 0.0, vp = 0.0;
        const bool ok = ud_point(c, uv[2 * i], uv[2 * i + 1], &up, &vp);
        out[2 * i] = ok ? up : 0.0;
        out[2 * i + 1] = ok ? vp : 0.0;
        flag[i] = ok ? 0 : 1;
    }
    return ECAL_OK;
}

// the camera, the options (null: not asked) and the event count of an entry point
static int undistort_check(ecal_ctx *ctx, const char *who, const ecal_undistort_camera *cam, const Options *o, uint64_t n_events) {
    if (const char *bad = ecal_undistort_camera_error(cam)) {
        ctx->last_error = std::string(who) + ": " + bad;
        return ECAL_ERR_INVALID;
    }
    if (o)
        if (const char *bad = ud_options_error(*o)) {
            ctx->last_error = std::string(who) + ": " + bad;
            return ECAL_ERR_INVALID;
        }
    return ecal_events_range_check(ctx, who, n_events);
}

extern "C" int ecal_undistort_points_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, const uint8_t *d_events, uint64_t n_events, double *d_uv,
                                         uint8_t *d_flag, void *stream) {
    const ecal_range range__(ctx, "ecal_undistort_points");
    if (!ctx) return ECAL_ERR_INVALID;
    if (n_events && (!d_events || !d_uv || !d_flag)) {
        ctx->last_error = "ecal_undistort_points: null pointer (events, uv or flag)";
        return ECAL_ERR_INVALID;
    }
    const int rc = undistort_check(ctx, "ecal_undistort_points", cam, nullptr, n_events);
    if (rc) return rc;
    if (!n_events) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    const uint32_t n = (uint32_t) n_events;
    hipLaunchKernelGGL(undistort_points_kernel, dim3((uint32_t) ((n_events + UD_T - 1) / UD_T)), dim3(UD_T), 0, st, ud_camera(cam), d_events, n, d_uv,
                       d_flag);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_undistort_events_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, const ecal_undistort_options *opt, const uint8_t *d_events,
                                         uint64_t n_events, uint8_t *d_out, uint32_t *d_count, ecal_undistort_totals *d_totals, void *stream) {
    const ecal_range range__(ctx, "ecal_undistort_events");
    if (!ctx) return ECAL_ERR_INVALID;
    if (!d_count || (n_events && (!d_events || !d_out))) {
        ctx->last_error = "ecal_undistort_events: null pointer (count, events or output)";
        return ECAL_ERR_INVALID;
    }
    const Options o = ud_options(opt);
    int rc = undistort_check(ctx, "ecal_undistort_events", cam, &o, n_events);
    if (rc) return rc;
    hipStream_t st = (hipStream_t) stream;
    if ((rc = ecal_compact_begin(ctx, "ecal_undistort_events", d_events, n_events, d_out, d_count, d_totals, sizeof(ecal_undistort_totals), st))) return rc;
    if (!n_events) return ECAL_OK;
    ecal_verdict_tables V;
    if ((rc = ecal_verdict_tables_ensure(ctx, ctx->undistort_scratch, n_events, &V))) return rc;
    const Camera c = ud_camera(cam);
    ecal_load_timer tm("undistort", ctx->sw.load_trace, st);
    tm.mark("start");
    hipLaunchKernelGGL(undistort_verdict_kernel, dim3(V.nb), dim3(UD_T), 0, st, c, o, d_events, n_events, V.verdict, V.cnt,
                       (unsigned long long *) d_totals);
    tm.mark("verdict");
    rc = ecal_compact_by_verdict(ctx, V, d_count, &tm, st, [&]() {
        hipLaunchKernelGGL(undistort_write_kernel, dim3(V.nb), dim3(UD_T), 0, st, c, o, d_events, n_events, (const uint8_t *) V.verdict,
                           (const uint32_t *) V.off, d_out);
    });
    if (rc) return rc;
    if (tm.on) ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (ECAL_TRACE=load alone: the timer reads its events when it goes out of scope)
    return ECAL_OK;
}

extern "C" int ecal_stream_undistort(ecal_ctx *ctx, const ecal_stream *in, const ecal_undistort_camera *cam, const ecal_undistort_options *opt,
                                     ecal_stream **out, ecal_undistort_totals *totals) {
    if (!ctx || !in || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    if (totals) memset(totals, 0, sizeof(*totals));
    const Options o = ud_options(opt);
    const uint64_t n = ecal_stream_size(in);
    int rc = undistort_check(ctx, "ecal_stream_undistort", cam, &o, n);
    if (rc) return rc;
    const uint8_t *d_in = ecal_stream_data(in);
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // totals | count
    rc = ecal_ensure(ctx, ctx->undistort_results, sizeof(ecal_undistort_totals) + 8);
    if (rc) return rc;
    ecal_undistort_totals T;
    return ecal_stream_compacted(
        ctx, "ecal_stream_undistort", in, ctx->undistort_results.ptr, &T, sizeof(T),
        [&](uint8_t *d_out, uint32_t *d_count, void *d_totals, hipStream_t st) {
            return ecal_undistort_events_dev(ctx, cam, opt, d_in, n, d_out, d_count, (ecal_undistort_totals *) d_totals, st);
        },
        [&](uint32_t kept, uint64_t n_in) -> const char * {
            if (totals) *totals = T;
            return T.n_kept != kept || T.n_invalid + T.n_outside + T.n_kept != n_in ? "the counters disagree" : nullptr;
        },
        out);
}

extern "C" int ecal_undistorted_frames_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, const ecal_undistort_options *opt, const double *d_xy,
                                           const ecal_packed_points *pk, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, uint32_t S,
                                           uint8_t *d_rgb, ecal_undistort_frame_totals *d_frame_totals, void *stream) {
    const ecal_range range__(ctx, "ecal_undistorted_frames");
    if (!ctx) return ECAL_ERR_INVALID;
    if (pk && (!pk->d_xy16 || !pk->d_seg_fmt)) pk = nullptr;
    if (S && (!d_seg_off || !d_seg_cnt || !d_rgb || (!d_xy && !pk))) {
        ctx->last_error = "ecal_undistorted_frames: null pointer (points, segments or picture)";
        return ECAL_ERR_INVALID;
    }
    const Options o = ud_options(opt);
    const int rc = undistort_check(ctx, "ecal_undistorted_frames", cam, &o, 0);
    if (rc) return rc;
    if (o.mode != UD_PIXEL) {
        ctx->last_error = "ecal_undistorted_frames: mode must be ECAL_UNDISTORT_PIXEL";
        return ECAL_ERR_INVALID;
    }
    if (!S) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    const uint32_t n_words = (uint32_t) (((uint64_t) o.out_width * o.out_height + UF_PIXELS_PER_WORD - 1) / UF_PIXELS_PER_WORD);
    const Camera c = ud_camera(cam);
    const uint32_t *xy16 = pk ? pk->d_xy16 : nullptr, *fmt = pk ? pk->d_seg_fmt : nullptr;
    if (n_words <= UF_LDS_WORDS) {
        hipLaunchKernelGGL(undistorted_frames_kernel<true>, dim3(S), dim3(UF_T), 0, st, c, o, d_xy, xy16, fmt, d_seg_off, d_seg_cnt, n_words,
                           (uint32_t *) nullptr, d_rgb, reinterpret_cast<FrameTotals *>(d_frame_totals));
    } else {
        const size_t bytes = (size_t) S * n_words * 4;
        const int erc = ecal_ensure(ctx, ctx->undistort_bits, bytes);
        if (erc) return erc;
        ECAL_HIP_TRY(ctx, hipMemsetAsync(ctx->undistort_bits.ptr, 0, bytes, st));
        hipLaunchKernelGGL(undistorted_frames_kernel<false>, dim3(S), dim3(UF_T), 0, st, c, o, d_xy, xy16, fmt, d_seg_off, d_seg_cnt, n_words,
                           ctx->undistort_bits.as<uint32_t>(), d_rgb, reinterpret_cast<FrameTotals *>(d_frame_totals));
    }
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_stream_undistorted_frames(ecal_ctx *ctx, const ecal_stream *es, const ecal_undistort_camera *cam,
                                              const ecal_undistort_options *opt, const double *t0, const double *t1, uint32_t S, uint8_t *rgb,
                                              ecal_undistort_frame_totals *totals) {
    if (!ctx || !es || (S && (!t0 || !t1 || !rgb))) return ECAL_ERR_INVALID;
    const Options o = ud_options(opt);
    int rc = undistort_check(ctx, "ecal_stream_undistorted_frames", cam, &o, 0);
    if (rc) return rc;
    if (o.mode != UD_PIXEL) {
        ctx->last_error = "ecal_stream_undistorted_frames: mode must be ECAL_UNDISTORT_PIXEL";
        return ECAL_ERR_INVALID;
    }
    if (!S) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t *d_events = ecal_stream_data(es);
    const uint64_t n_events = ecal_stream_size(es);
    ecal_det_scratch &det = ctx->det;
    // 1. the windows' event ranges; their sum is the slicer's capacity
    if ((rc = ecal_det_ensure_bounds(ctx, S))) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(det.t0(), t0, S * sizeof(double), hipMemcpyHostToDevice, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(det.t1(), t1, S * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = ecal_window_bounds_dev(ctx, d_events, n_events, det.t0(), det.t1(), S, det.win_lo.as<uint32_t>(), det.win_hi.as<uint32_t>(),
                                     det.win_base.as<uint32_t>(), st)))
        return rc;
    uint32_t cap_points = 0;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(&cap_points, det.win_base.as<uint32_t>() + S, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    // 2. the slicer (the EventFrame constructor), doubles
    if (!cap_points) cap_points = 1;   // (no window holds an event: a capacity all the same)
    const size_t cap = (size_t) cap_points + 16;
    if ((rc = ecal_ensure(ctx, det.xy, cap * 16)) || (rc = ecal_ensure(ctx, det.seg_off, 2ul * S * 4)) ||
        (rc = ecal_ensure(ctx, det.seg_cnt, 2ul * S * 4)) || (rc = ecal_ensure(ctx, det.overflow, 16)))
        return rc;
    if ((rc = ecal_slice_events_dev(ctx, d_events, n_events, det.win_lo.as<uint32_t>(), det.win_hi.as<uint32_t>(), det.win_base.as<uint32_t>(), S, 0,
                                    cap_points, det.xy.as<double>(), det.seg_off.as<uint32_t>(), det.seg_cnt.as<uint32_t>(), nullptr,
                                    det.overflow.as<int>(), st)))
        return rc;
    // 3. the pictures | the totals
    const size_t pic = (size_t) o.out_width * o.out_height * 3, o_tot = (pic * S + 15) / 16 * 16;
    if ((rc = ecal_ensure(ctx, ctx->undistort_frames, o_tot + (size_t) S * sizeof(ecal_undistort_frame_totals)))) return rc;
    uint8_t *d_rgb = ctx->undistort_frames.as<uint8_t>();
    ecal_undistort_frame_totals *d_tot = reinterpret_cast<ecal_undistort_frame_totals *>(d_rgb + o_tot);
    if ((rc = ecal_undistorted_frames_dev(ctx, cam, opt, det.xy.as<double>(), nullptr, det.seg_off.as<uint32_t>(), det.seg_cnt.as<uint32_t>(), S, d_rgb,
                                          d_tot, st)))
        return rc;
    int overflow = 0;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(&overflow, det.overflow.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(rgb, d_rgb, pic * S, hipMemcpyDeviceToHost, st));
    if (totals) ECAL_HIP_TRY(ctx, hipMemcpyAsync(totals, d_tot, (size_t) S * sizeof(ecal_undistort_frame_totals), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (overflow) {
        ctx->last_error = "ecal_stream_undistorted_frames: the slicer's capacity was exceeded";
        return ECAL_ERR_HIP;
    }
    return ECAL_OK;
}
