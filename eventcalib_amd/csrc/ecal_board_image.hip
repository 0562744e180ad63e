// Board-frame event image (include/ecal.h, ecal_solver_board_image[_dev] / ecal_solver_board_points[_dev]): every raw event of
// the stream carried through the solved intrinsics and the pose of the spline at its own time stamp onto the calibration board —
// the motion-compensated image of event-camera work.  The quality report (ecal_report.hip) sees only the events the association
// kept, and the keyframes made that choice; this pass sees all of them.
//
// The reference's only picture of a result is EventFrame::undistortedImage (event/src/EventFrame.cpp:38-60): one window's
// undistorted pixels, red for positive and green for negative events, no pose and no time.  This is new functionality in its place.
//
// One streaming pass over the packed 25-byte records, a block of ECAL_BOARD_IMAGE_BLOCK consecutive events per workgroup.  The
// stream is time-sorted, so a block meets a handful of consecutive knot spans of one segment: its first and last span are
// found once per workgroup (waves 0 and 1, as report_kernel finds its keyframe interval) and their control points and knots are
// staged in LDS; a block that meets more than ECAL_BOARD_IMAGE_CP_LDS control points or more than one segment reads them from
// global memory per event instead.  The image is one global u32 atomic per event; the ring profile lives in LDS and leaves the
// workgroup once, non-empty bins only.  Design, LDS budget, atomics per event: design/08_solver.md §"Board image".
//
// Floating point: the board point is compiled as the solver compiles its residual (contraction to FMA allowed, the pragma around
// the include); everything that decides a BIN (pixel, nearest landmark, ring range, ring bin) is compiled without contraction,
// the file's default.
#include <hip/hip_runtime.h>
#pragma clang fp contract(fast)
#include "spline_residual.hpp"
#pragma clang fp contract(off)
#include "ecal_solver_state.hpp"
#include "block_utils.hpp"
#include "board_nearest.hpp"
#include "board_block.hpp"

#include <algorithm>

namespace ecal {

constexpr uint32_t BI_MAX_RING = 256;
constexpr uint32_t BI_NTOT = 7;   // words of ecal_board_image_totals

struct BoardArgs {
    uint32_t n_lm;
    double x0, y0, bin;
    uint32_t width, height, ring_bins;
    double ring_range, radius;
    uint32_t *img;
    unsigned long long *totals;
    ecal_ring_stats *ring_stats;
    unsigned long long *ring_hist;
    double *xw;       // the per-event form
    uint8_t *flag;
};

// (the block's plan and the per-event pose fetch: board_block.hpp, shared with ecal_reassociate.hip)

template <bool SO3, bool FISHEYE, bool POINTS>
__global__ __launch_bounds__(BI_T, 2) void board_image_kernel(const uint8_t *__restrict__ rec, uint64_t n_events,
                                                          const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                          const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                          const double *__restrict__ seg_range, uint32_t n_seg, uint32_t n_cp_total,
                                                          const double *__restrict__ landmarks, const BoardArgs A) {
    const BoardSpline S{knots, knot_off, cp_off, params, seg_range, n_seg, n_cp_total};
    extern __shared__ __attribute__((aligned(16))) double dyn[];   // landmarks [n_lm][2] | ring sums [2][n_lm][2] | ring counts [n_lm][2] | ring hist
    __shared__ BoardBlockLds s_blk;
    __shared__ uint32_t s_red[(BI_T / 64) * BI_NTOT];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * BI_BLOCK;
    const uint32_t count = (uint32_t) (n_events - base < (uint64_t) BI_BLOCK ? n_events - base : (uint64_t) BI_BLOCK);
    const uint8_t *const blk = rec + base * 25;
    const bool ring = !POINTS && A.ring_bins != 0;
    const uint32_t n_lm = ring ? A.n_lm : 0u, n_hist = n_lm * A.ring_bins;
    double *const s_lm = dyn, *const s_rsum = dyn + 2 * (size_t) n_lm;
    uint32_t *const s_rcnt = reinterpret_cast<uint32_t *>(s_rsum + 4 * (size_t) n_lm), *const s_hist = s_rcnt + 2 * (size_t) n_lm;
    if (ring) {
        for (uint32_t i = (uint32_t) tid; i < n_lm; i += BI_T) {
            s_lm[2 * i] = landmarks[3 * (size_t) i];
            s_lm[2 * i + 1] = landmarks[3 * (size_t) i + 1];
        }
        for (uint32_t i = (uint32_t) tid; i < 4 * n_lm; i += BI_T) s_rsum[i] = 0.0;
        for (uint32_t i = (uint32_t) tid; i < 2 * n_lm + n_hist; i += BI_T) s_rcnt[i] = 0u;
    }
    const BoardBlockPlan P = board_block_plan(blk, count, S, s_blk);   // (its barriers also publish the ring's LDS)

    double pin[9];
    for (int i = 0; i < 9; i++) pin[i] = params[i];
    const double ifx = 1.0 / pin[0], ify = 1.0 / pin[1];
    const double w_lim = (double) A.width, h_lim = (double) A.height;
    const double ring_den = __dmul_rn(2.0, A.ring_range), ring_top = (double) (A.ring_bins ? A.ring_bins - 1u : 0u);
    const size_t plane = (size_t) A.width * A.height;
    uint32_t tot[BI_NTOT] = {0, 0, 0, 0, 0, 0, 0};   // n_events, n_outside_time, n_behind, n_outside_image, n_image[2], n_ring

    for (uint32_t k = (uint32_t) tid; k < count; k += BI_T) {
        const uint8_t *r = blk + (size_t) k * 25;
        const double et = bi_load_f64(r), eu = bi_load_f64(r + 8), ev = bi_load_f64(r + 16);
        const uint32_t pol = r[24] ? 1u : 0u;
        tot[0]++;
        double q[4][4], t[4][3], b[4];
        const bool in_time = board_event_pose(P, S, s_blk, et, b, q, t);
        double Xw[2] = {0.0, 0.0};
        bool ok = false;
        if (in_time) {
            double Q[4], T[3];
            if (SO3) spline_pose_so3(b, q, t, Q, T); else spline_pose_quat(b, q, t, Q, T);
            ok = spline_board_point<FISHEYE>(eu, ev, pin, ifx, ify, Q[0], Q[1], Q[2], Q[3], T, Xw);
        }
        if (POINTS) {
            const uint64_t i = base + k;
            A.xw[2 * i] = ok ? Xw[0] : 0.0;
            A.xw[2 * i + 1] = ok ? Xw[1] : 0.0;
            A.flag[i] = !in_time ? (uint8_t) 1 : (ok ? (uint8_t) 0 : (uint8_t) 2);
            continue;
        }
        if (!in_time) {
            tot[1]++;
            continue;
        }
        if (!ok) {
            tot[2]++;
            continue;
        }
        const double fx = floor(__ddiv_rn(__dsub_rn(Xw[0], A.x0), A.bin)), fy = floor(__ddiv_rn(__dsub_rn(Xw[1], A.y0), A.bin));
        if (fx >= 0.0 && fx < w_lim && fy >= 0.0 && fy < h_lim) {          // (a NaN is outside)
            tot[4 + pol]++;
            if (A.img) atomicAdd(&A.img[pol * plane + (size_t) (uint32_t) fy * A.width + (uint32_t) fx], 1u);
        } else {
            tot[3]++;
        }
        if (ring) {
            double best;
            const uint32_t bi = board_nearest(s_lm, n_lm, Xw[0], Xw[1], &best);
            const double d = __dsqrt_rn(best) - A.radius;
            if (fabs(d) < A.ring_range) {
                double hb = floor(__ddiv_rn(__dmul_rn(__dadd_rn(d, A.ring_range), (double) A.ring_bins), ring_den));
                hb = hb > 0.0 ? hb : 0.0;
                hb = hb < ring_top ? hb : ring_top;
                tot[6]++;
                atomicAdd(&s_hist[bi * A.ring_bins + (uint32_t) hb], 1u);
                atomicAdd(&s_rcnt[2 * bi + pol], 1u);
                atomicAdd(&s_rsum[2 * bi + pol], d);
                atomicAdd(&s_rsum[2 * n_lm + 2 * bi + pol], __dmul_rn(d, d));
            }
        }
    }
    if (POINTS) return;

    // totals: per wave, then one atomic per workgroup and field
    for (int o = 32; o > 0; o >>= 1)
        for (uint32_t i = 0; i < BI_NTOT; i++) tot[i] += __shfl_down(tot[i], o, 64);
    if ((tid & 63) == 0)
        for (uint32_t i = 0; i < BI_NTOT; i++) s_red[(tid >> 6) * BI_NTOT + i] = tot[i];
    __syncthreads();   // ... and every thread's LDS bins are complete
    if ((uint32_t) tid < BI_NTOT) {
        uint32_t v = 0;
        for (int w = 0; w < BI_T / 64; w++) v += s_red[w * BI_NTOT + tid];
        if (v) atomicAdd(&A.totals[tid], (unsigned long long) v);
    }
    if (ring) {
        if (A.ring_hist)
            for (uint32_t i = (uint32_t) tid; i < n_hist; i += BI_T) {
                const uint32_t n = s_hist[i];
                if (n) atomicAdd(&A.ring_hist[i], (unsigned long long) n);
            }
        if (A.ring_stats)
            for (uint32_t i = (uint32_t) tid; i < 2 * n_lm; i += BI_T) {
                const uint32_t n = s_rcnt[i];
                if (!n) continue;
                atomicAdd((unsigned long long *) &A.ring_stats[i].n, (unsigned long long) n);
                atomicAdd(&A.ring_stats[i].sum_d, s_rsum[i]);
                atomicAdd(&A.ring_stats[i].sum_d2, s_rsum[2 * n_lm + i]);
            }
    }
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_board_image_totals) == 8 * BI_NTOT && sizeof(ecal_ring_stats) == 24, "the board image's records have no padding");

extern "C" int ecal_board_image_default_options(const ecal_solver *s, ecal_board_image_options *o) {
    if (!s || !o) return ECAL_ERR_INVALID;
    const double r = s->radius;
    double x_lo = 0.0, x_hi = 0.0, y_lo = 0.0, y_hi = 0.0;
    for (uint32_t i = 0; i < s->n_lm; i++) {
        const double x = s->landmarks[3 * (size_t) i], y = s->landmarks[3 * (size_t) i + 1];
        x_lo = i ? std::min(x_lo, x) : x;
        x_hi = i ? std::max(x_hi, x) : x;
        y_lo = i ? std::min(y_lo, y) : y;
        y_hi = i ? std::max(y_hi, y) : y;
    }
    o->x0 = x_lo - 3.0 * r;
    o->y0 = y_lo - 3.0 * r;
    o->bin = r / 8.0;
    const double w = ceil((x_hi - x_lo + 6.0 * r) / o->bin), h = ceil((y_hi - y_lo + 6.0 * r) / o->bin);
    o->width = w >= 1.0 && w < 4294967296.0 ? (uint32_t) w : 1u;    // (radius <= 0: the call refuses bin <= 0)
    o->height = h >= 1.0 && h < 4294967296.0 ? (uint32_t) h : 1u;
    o->ring_bins = 64;
    o->ring_range = r;
    return ECAL_OK;
}

// the options in force and their checks, shared by the device and the host form
static int board_options(ecal_solver *s, const ecal_board_image_options *opt_in, ecal_board_image_options *opt) {
    ecal_ctx *ctx = s->ctx;
    if (opt_in) *opt = *opt_in; else (void) ecal_board_image_default_options(s, opt);
    if (!(opt->bin > 0.0) || !(opt->bin <= 1.79769313486231570e308) || !(fabs(opt->x0) <= 1.79769313486231570e308) ||
        !(fabs(opt->y0) <= 1.79769313486231570e308)) {
        ctx->last_error = "ecal_solver_board_image: bin > 0 and a finite origin";
        return ECAL_ERR_INVALID;
    }
    if ((uint64_t) opt->width * opt->height > (1ull << 24)) {
        ctx->last_error = "ecal_solver_board_image: width * height <= 2^24";
        return ECAL_ERR_RANGE;
    }
    if (opt->ring_bins > BI_MAX_RING || (opt->ring_bins && !(opt->ring_range > 0.0 && opt->ring_range <= 1.79769313486231570e308))) {
        ctx->last_error = "ecal_solver_board_image: ring_bins <= 256 and a positive ring_range";
        return ECAL_ERR_INVALID;
    }
    if (opt->ring_bins && s->n_lm > BI_MAX_LM) {
        ctx->last_error = "ecal_solver_board_image: the ring profile takes at most 128 landmarks";
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

template <bool POINTS>
static int board_launch(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events, const BoardArgs &A, size_t lds,
                        hipStream_t st) {
    ecal_ctx *ctx = s->ctx;
    const void *fn = s->use_so3 ? (s->fisheye ? (const void *) &board_image_kernel<true, true, POINTS> : (const void *) &board_image_kernel<true, false, POINTS>)
                                : (s->fisheye ? (const void *) &board_image_kernel<false, true, POINTS> : (const void *) &board_image_kernel<false, false, POINTS>);
    if (lds > s->board_lds) {
        ECAL_HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        s->board_lds = lds;
    }
    const uint32_t nb = (uint32_t) ((n_events + BI_BLOCK - 1) / BI_BLOCK);
#define ECAL_BI_LAUNCH(SO3_, FISH_)                                                                                                \
    hipLaunchKernelGGL((board_image_kernel<SO3_, FISH_, POINTS>), dim3(nb), dim3(BI_T), lds, st, d_events, n_events, s->d_knots,       \
                       s->d_knot_off, s->d_cp_off, d_params, s->d_seg_range, s->n_seg, s->n_cp, s->d_landmarks, A)
    if (s->use_so3) {
        if (s->fisheye) ECAL_BI_LAUNCH(true, true); else ECAL_BI_LAUNCH(true, false);
    } else {
        if (s->fisheye) ECAL_BI_LAUNCH(false, true); else ECAL_BI_LAUNCH(false, false);
    }
#undef ECAL_BI_LAUNCH
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_solver_board_image_dev(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events,
                                           const ecal_board_image_options *opt_in, uint32_t *d_img, ecal_board_image_totals *d_totals,
                                           ecal_ring_stats *d_ring_stats, uint64_t *d_ring_hist, void *stream) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_board_image");
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!d_params || !d_totals || (n_events && !d_events)) {
        ctx->last_error = "ecal_solver_board_image: null pointer (parameters, totals or events)";
        return ECAL_ERR_INVALID;
    }
    if (n_events > 0xFFFFFFFFull) {
        ctx->last_error = "ecal_solver_board_image: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    ecal_board_image_options opt;
    const int rc = board_options(s, opt_in, &opt);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    const size_t plane = (size_t) opt.width * opt.height;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_totals, 0, sizeof(ecal_board_image_totals), st));
    if (d_img && plane) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_img, 0, 2 * plane * sizeof(uint32_t), st));
    if (d_ring_stats && s->n_lm) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_ring_stats, 0, 2 * (size_t) s->n_lm * sizeof(ecal_ring_stats), st));
    if (d_ring_hist && s->n_lm && opt.ring_bins)
        ECAL_HIP_TRY(ctx, hipMemsetAsync(d_ring_hist, 0, (size_t) s->n_lm * opt.ring_bins * sizeof(uint64_t), st));
    if (!n_events) return ECAL_OK;
    BoardArgs A{};
    A.n_lm = s->n_lm;
    A.x0 = opt.x0;
    A.y0 = opt.y0;
    A.bin = opt.bin;
    A.width = opt.width;
    A.height = opt.height;
    A.ring_bins = opt.ring_bins;
    A.ring_range = opt.ring_range;
    A.radius = s->radius;
    A.img = d_img;
    A.totals = (unsigned long long *) d_totals;
    A.ring_stats = d_ring_stats;
    A.ring_hist = (unsigned long long *) d_ring_hist;
    // landmarks 16 B, ring sums 32 B and counts 8 B per landmark, 4 B per histogram bin: <= 135 KB of the CU's 160
    const size_t lds = opt.ring_bins ? (size_t) s->n_lm * 56 + (size_t) s->n_lm * opt.ring_bins * 4 : 0;
    return board_launch<false>(s, d_params, d_events, n_events, A, lds, st);
}

extern "C" int ecal_solver_board_points_dev(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events,
                                            double *d_xw, uint8_t *d_flag, void *stream) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_board_points");
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!d_params || (n_events && (!d_events || !d_xw || !d_flag))) {
        ctx->last_error = "ecal_solver_board_points: null pointer (parameters, events or outputs)";
        return ECAL_ERR_INVALID;
    }
    if (n_events > 0xFFFFFFFFull) {
        ctx->last_error = "ecal_solver_board_points: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    if (!n_events) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BoardArgs A{};
    A.n_lm = s->n_lm;
    A.xw = d_xw;
    A.flag = d_flag;
    return board_launch<true>(s, d_params, d_events, n_events, A, 0, (hipStream_t) stream);
}

extern "C" int ecal_solver_board_image(ecal_solver *s, const double *params, const ecal_stream *es, const ecal_board_image_options *opt_in,
                                       uint32_t *img, ecal_board_image_totals *totals, ecal_ring_stats *ring_stats, uint64_t *ring_hist) {
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!params || !es || !totals) {
        ctx->last_error = "ecal_solver_board_image: null pointer (parameters, stream or totals)";
        return ECAL_ERR_INVALID;
    }
    ecal_board_image_options opt;
    int rc = board_options(s, opt_in, &opt);
    if (rc) return rc;
    // the device images of the outputs, one after another in the context's scratch (sizes in 8-byte words)
    const size_t plane = (size_t) opt.width * opt.height;
    const size_t w_tot = BI_NTOT, w_rs = ring_stats ? 6 * (size_t) s->n_lm : 0, w_rh = ring_hist ? (size_t) s->n_lm * opt.ring_bins : 0,
                 w_img = img ? plane : 0;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    rc = ecal_ensure(ctx, ctx->board_scratch, (w_tot + w_rs + w_rh + w_img) * 8);
    if (rc) return rc;
    uint64_t *p_tot = ctx->board_scratch.as<uint64_t>(), *p_rs = p_tot + w_tot, *p_rh = p_rs + w_rs, *p_img = p_rh + w_rh;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    rc = ecal_solver_board_image_dev(s, s->d_params, ecal_stream_data(es), ecal_stream_size(es), &opt, w_img ? (uint32_t *) p_img : nullptr,
                                     (ecal_board_image_totals *) p_tot, w_rs ? (ecal_ring_stats *) p_rs : nullptr, w_rh ? p_rh : nullptr, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(totals, p_tot, w_tot * 8, hipMemcpyDeviceToHost, st));
    if (w_rs) ECAL_HIP_TRY(ctx, hipMemcpyAsync(ring_stats, p_rs, w_rs * 8, hipMemcpyDeviceToHost, st));
    if (w_rh) ECAL_HIP_TRY(ctx, hipMemcpyAsync(ring_hist, p_rh, w_rh * 8, hipMemcpyDeviceToHost, st));
    if (w_img) ECAL_HIP_TRY(ctx, hipMemcpyAsync(img, p_img, w_img * 8, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}

extern "C" int ecal_solver_board_points(ecal_solver *s, const double *params, const ecal_stream *es, double *xw, uint8_t *flag) {
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!params || !es) {
        ctx->last_error = "ecal_solver_board_points: null pointer (parameters or stream)";
        return ECAL_ERR_INVALID;
    }
    const uint64_t n = ecal_stream_size(es);
    if (!n) return ECAL_OK;
    if (!xw || !flag) {
        ctx->last_error = "ecal_solver_board_points: null pointer (outputs)";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ecal_ensure(ctx, ctx->board_scratch, (size_t) n * 17);
    if (rc) return rc;
    double *p_xw = ctx->board_scratch.as<double>();
    uint8_t *p_flag = reinterpret_cast<uint8_t *>(p_xw + 2 * n);
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    rc = ecal_solver_board_points_dev(s, s->d_params, ecal_stream_data(es), n, p_xw, p_flag, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(xw, p_xw, (size_t) n * 16, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(flag, p_flag, (size_t) n, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}
