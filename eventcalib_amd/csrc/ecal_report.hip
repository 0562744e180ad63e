// Calibration quality report: the raw residuals of the solver's problem binned per keyframe, per landmark, per sensor cell
// and into a histogram, in ONE pass over the residual records (include/ecal.h, ecal_solver_report[_dev]).
//
// The reference prints an RMS after its init stage (event_camera_calib/src/EventCalibIni.cpp:202-209) and Ceres' FullReport
// after the solve; neither says which keyframe, which circle or which part of the sensor fits badly.  The seam that did exist,
// ecal_residuals, writes one double per residual (360 MB at 45 M residuals) for a host to bin.  Here the records never leave
// HBM: one workgroup per chunk as in the normal-equation kernel, the residual arithmetic of spline_residual.hpp without the
// Jacobian, and a few kilobytes of output.  Design, LDS budget and atomic counts: design/08_solver.md §"Quality report".
//
// Floating point: the residual code is compiled as the solver compiles it (contraction to FMA allowed, the pragma around the
// include below), so r is the value the cost kernel sees; everything that decides a BIN (keyframe tie rule, cell, histogram
// bin, outlier threshold) is compiled without contraction, the file's default, and comes out the same on any build.
#include <hip/hip_runtime.h>
#pragma clang fp contract(fast)
#include "spline_residual.hpp"
#pragma clang fp contract(off)
#include "ecal_solver_state.hpp"
#include "block_utils.hpp"
#include "report_bins.hpp"

#include <algorithm>

namespace ecal {

struct ReportArgs {
    const double *kf_time;
    uint32_t n_kf, n_lm;
    uint32_t cell_px, cells_x, cells_y, n_cells;   // n_cells = 0: no coverage map
    uint32_t hist_bins;                            // 0: no histogram
    double hist_range, outlier;
    ecal_report_totals *total;
    ecal_bin_stats *kf, *lm;                       // NULL: family skipped
    unsigned long long *cell_n, *hist;
    double *cell_sum_r2;
};

// One workgroup per chunk.  Totals live in registers; the keyframe of a thread's residuals never decreases along the chunk
// (records are time-sorted), so a thread keeps ONE keyframe's statistics in registers and hands them to the workgroup's LDS bins
// when its keyframe changes — a handful of times per chunk; landmark, cell and histogram bins are LDS atomics per residual.
// Everything leaves the workgroup once, at the end, bins that stayed empty not at all.
template <bool SO3, bool FISHEYE>
__global__ __launch_bounds__(NE_T) void report_kernel(const ResRecord *__restrict__ rec, const Chunk *__restrict__ chunks,
                                                     const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                     const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                     uint32_t n_cp_total, const double *__restrict__ landmarks, double radius,
                                                     double huber_a, const ReportArgs A) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];   // lm sums [4][n_lm] | cell sums [n_cells] | lm counts [2][n_lm] | cell counts | hist
    __shared__ double s_kt[RP_KF_LDS], s_kfsum[3 * RP_KF_LDS], s_red[5 * (NE_T / 64)];
    __shared__ unsigned long long s_kfmax[RP_KF_LDS];
    __shared__ uint32_t s_kfcnt[2 * RP_KF_LDS], s_redn[2 * (NE_T / 64)], s_bounds[2];
    const Chunk ch = chunks[blockIdx.x];
    const int tid = threadIdx.x;
    const bool want_kf = A.kf != nullptr, want_lm = A.lm != nullptr;
    const uint32_t n_lm = want_lm ? A.n_lm : 0u, n_cells = A.n_cells, n_hist = A.hist_bins;
    double *const lm_sum = dyn, *const cell_sum = dyn + 4 * (size_t) n_lm;
    uint32_t *const lm_cnt = reinterpret_cast<uint32_t *>(cell_sum + n_cells), *const cell_cnt = lm_cnt + 2 * (size_t) n_lm,
                    *const hist = cell_cnt + n_cells;
    const LdsBins lmb{lm_cnt, lm_sum, reinterpret_cast<unsigned long long *>(lm_sum + 3 * (size_t) n_lm), n_lm},
        kfb{s_kfcnt, s_kfsum, s_kfmax, RP_KF_LDS};
    {
        const uint32_t dyn_words = 8 * n_lm + 2 * n_cells + 2 * n_lm + n_cells + n_hist;
        uint32_t *w = reinterpret_cast<uint32_t *>(dyn);
        for (uint32_t i = (uint32_t) tid; i < dyn_words; i += NE_T) w[i] = 0u;
        for (uint32_t i = (uint32_t) tid; i < 3 * RP_KF_LDS; i += NE_T) s_kfsum[i] = 0.0;
        for (uint32_t i = (uint32_t) tid; i < RP_KF_LDS; i += NE_T) s_kfmax[i] = 0ull;
        for (uint32_t i = (uint32_t) tid; i < 2 * RP_KF_LDS; i += NE_T) s_kfcnt[i] = 0u;
    }
    // the chunk's keyframe interval, once per workgroup: the lower bounds of its first and last time (waves 0 and 1)
    const uint32_t K = A.n_kf;
    if (want_kf && tid < 128) {
        const double tq = rec[ch.start + ((tid >> 6) ? ch.count - 1u : 0u)].t;
        const uint32_t a = wave_lower_bound(A.kf_time, K, tq);
        if ((tid & 63) == 0) s_bounds[tid >> 6] = a;
    }
    __syncthreads();
    uint32_t a_lo = 0, a_hi = 0, k_first = 0, n_bins = 0;
    bool staged = false;
    if (want_kf) {
        a_lo = s_bounds[0];
        a_hi = s_bounds[1];
        k_first = a_lo > 0 ? a_lo - 1u : 0u;                      // the residuals' keyframes lie in [k_first, min(a_hi, K - 1)]
        n_bins = (a_hi < K ? a_hi : K - 1u) - k_first + 1u;
        staged = n_bins <= RP_KF_LDS;
        if (staged && (uint32_t) tid < n_bins) s_kt[tid] = A.kf_time[k_first + tid];
    }
    __syncthreads();

    const double *kn = knots + knot_off[ch.seg];
    const uint32_t c0 = cp_off[ch.seg] + ch.span - 3;
    const double *qall = params + 9;
    const double *tall = params + 9 + 4 * (size_t) n_cp_total;
    double q[4][4], t[4][3], pin[9], binv[6];
    for (int i = 0; i < 9; i++) pin[i] = params[i];
    spline_span_inverses(kn, ch.span, binv);
    const double ifx = 1.0 / pin[0], ify = 1.0 / pin[1], inv_huber_a = 1.0 / huber_a;
    for (int j = 0; j < 4; j++) {
        for (int k = 0; k < 4; k++) q[j][k] = qall[4 * (size_t) (c0 + j) + k];
        for (int k = 0; k < 3; k++) t[j][k] = tall[3 * (size_t) (c0 + j) + k];
    }
    const double hist_scale_den = __dmul_rn(2.0, A.hist_range), hist_top = (double) (n_hist ? n_hist - 1u : 0u);

    BinAcc tot, cur;          // the chunk's totals; the statistics of keyframe cur_k
    uint32_t cur_k = 0;
    double cost = 0.0;
    auto kf_hand_over = [&]() {
        if (!cur.n) return;
        if (staged) kfb.add(cur_k - k_first, cur);
        else bin_add_global(A.kf + cur_k, cur);   // a chunk across more keyframes than the LDS bins hold (a sparse stream)
        cur = BinAcc();
    };

    // (the next record is asked for before this one's residual is evaluated, as in normal_eq_kernel)
    ResRecord e_next = rec[ch.start + min((uint32_t) tid, ch.count - 1u)];
    for (uint32_t k = (uint32_t) tid; k < ch.count; k += NE_T) {
        const ResRecord e = e_next;
        e_next = rec[ch.start + min(k + (uint32_t) NE_T, ch.count - 1u)];
        ResidualInput in;
        residual_input_fill(in, e, landmarks, radius, ifx, ify, kn, ch.span, binv);
        const double r = SO3 ? spline_residual_so3<FISHEYE>(in, pin, q, t, nullptr) : spline_residual<FISHEYE>(in, pin, q, t, nullptr);
        double hr = 0.0;
        (void) huber_scale(r, huber_a, &hr, inv_huber_a);
        cost += hr;
        const double ar = fabs(r), r2 = __dmul_rn(r, r);
        const bool out = ar > A.outlier;
        tot.add(r, ar, r2, out);
        if (want_kf) {
            const uint32_t kf = staged ? nearest_keyframe(s_kt, k_first, K, a_lo, a_hi, e.t) : nearest_keyframe(A.kf_time, 0u, K, a_lo, a_hi, e.t);
            if (kf != cur_k) {
                kf_hand_over();
                cur_k = kf;
            }
            cur.add(r, ar, r2, out);
        }
        if (want_lm) {
            BinAcc one;
            one.add(r, ar, r2, out);
            lmb.add(e.lm, one);
        }
        if (n_cells) {
            // (uint32) max(u, 0) / cell_px, the last column / row taking what lies beyond the sensor
            const uint32_t px = (uint32_t) fmin(fmax(e.u, 0.0), 4294967040.0), py = (uint32_t) fmin(fmax(e.v, 0.0), 4294967040.0);
            const uint32_t cx = min(px / A.cell_px, A.cells_x - 1u), cy = min(py / A.cell_px, A.cells_y - 1u);
            const uint32_t c = cy * A.cells_x + cx;
            atomicAdd(&cell_cnt[c], 1u);
            atomicAdd(&cell_sum[c], r2);
        }
        if (n_hist) {
            double b = floor(__ddiv_rn(__dmul_rn(__dadd_rn(r, A.hist_range), (double) n_hist), hist_scale_den));
            b = b > 0.0 ? b : 0.0;             // (a NaN residual counts in bin 0)
            b = b < hist_top ? b : hist_top;
            atomicAdd(&hist[(uint32_t) b], 1u);
        }
    }
    kf_hand_over();

    // totals: wave reduction, then one thread adds the workgroup's seven numbers and two counts
    {
        double v[5] = {tot.sum_r, tot.sum_r2, tot.sum_abs, cost, tot.max_abs};
        uint32_t c[2] = {tot.n, tot.n_out};
        for (int o = 32; o > 0; o >>= 1) {
            for (int i = 0; i < 4; i++) v[i] += __shfl_down(v[i], o, 64);
            v[4] = fmax(v[4], __shfl_down(v[4], o, 64));
            for (int i = 0; i < 2; i++) c[i] += __shfl_down(c[i], o, 64);
        }
        if ((tid & 63) == 0) {
            for (int i = 0; i < 5; i++) s_red[5 * (tid >> 6) + i] = v[i];
            for (int i = 0; i < 2; i++) s_redn[2 * (tid >> 6) + i] = c[i];
        }
    }
    __syncthreads();   // ... and every thread's LDS bins are complete
    if (tid == 0) {
        BinAcc a;
        double cs = 0.0;
        for (int w = 0; w < NE_T / 64; w++) {
            a.sum_r += s_red[5 * w];
            a.sum_r2 += s_red[5 * w + 1];
            a.sum_abs += s_red[5 * w + 2];
            cs += s_red[5 * w + 3];
            a.max_abs = fmax(a.max_abs, s_red[5 * w + 4]);
            a.n += s_redn[2 * w];
            a.n_out += s_redn[2 * w + 1];
        }
        bin_add_global(&A.total->all, a);
        atomicAdd(&A.total->cost, cs);
    }
    if (staged) kfb.flush(A.kf, k_first, n_bins, tid);
    if (want_lm) lmb.flush(A.lm, 0u, n_lm, tid);
    for (uint32_t i = (uint32_t) tid; i < n_cells; i += NE_T) {
        const uint32_t n = cell_cnt[i];
        if (!n) continue;
        if (A.cell_n) atomicAdd(&A.cell_n[i], (unsigned long long) n);
        if (A.cell_sum_r2) atomicAdd(&A.cell_sum_r2[i], cell_sum[i]);
    }
    for (uint32_t i = (uint32_t) tid; i < n_hist; i += NE_T) {
        const uint32_t n = hist[i];
        if (n) atomicAdd(&A.hist[i], (unsigned long long) n);
    }
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_bin_stats) == 48 && sizeof(ecal_report_totals) == 56, "the report's records have no padding");

extern "C" uint32_t ecal_solver_num_landmarks(const ecal_solver *s) { return s ? s->n_lm : 0; }

extern "C" void ecal_report_default_options(ecal_report_options *o) {
    if (!o) return;
    o->width = 346;   // the reference's sensor (DAVIS346)
    o->height = 260;
    o->cell_px = 16;
    o->hist_bins = 64;
    o->hist_range = 0.0;       // 4 * huber_a, filled in by the call
    o->outlier_thresh = 0.0;   // huber_a
}

extern "C" int ecal_solver_report_dev(ecal_solver *s, const double *d_params, const double *d_kf_time, uint32_t n_keyframes,
                                      const ecal_report_options *opt_in, ecal_report_totals *d_total, ecal_bin_stats *d_kf,
                                      ecal_bin_stats *d_lm, uint64_t *d_cell_n, double *d_cell_sum_r2, uint64_t *d_hist, void *stream) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_report");
    if (!s || !d_params || !d_total) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ecal_report_options opt;
    if (opt_in) opt = *opt_in; else ecal_report_default_options(&opt);
    ReportArgs A{};
    A.total = d_total;
    A.outlier = opt.outlier_thresh > 0.0 ? opt.outlier_thresh : s->huber_a;
    if (d_kf) {
        if (!d_kf_time || n_keyframes == 0) {
            ctx->last_error = "ecal_solver_report: per-keyframe statistics need a keyframe table";
            return ECAL_ERR_INVALID;
        }
        A.kf = d_kf;
        A.kf_time = d_kf_time;
        A.n_kf = n_keyframes;
    }
    if (d_lm) {
        if (s->n_lm > RP_MAX_LM) {
            ctx->last_error = "ecal_solver_report: per-landmark statistics for at most 1024 landmarks";
            return ECAL_ERR_RANGE;
        }
        A.lm = d_lm;
        A.n_lm = s->n_lm;
    }
    if (d_cell_n || d_cell_sum_r2) {
        if (opt.cell_px == 0 || opt.width == 0 || opt.height == 0) {
            ctx->last_error = "ecal_solver_report: the coverage map needs width, height and cell_px > 0";
            return ECAL_ERR_INVALID;
        }
        const uint64_t cx = ((uint64_t) opt.width + opt.cell_px - 1) / opt.cell_px, cy = ((uint64_t) opt.height + opt.cell_px - 1) / opt.cell_px;
        if (cx * cy > RP_MAX_CELLS) {
            ctx->last_error = "ecal_solver_report: more than 8192 coverage cells";
            return ECAL_ERR_INVALID;
        }
        A.cell_px = opt.cell_px;
        A.cells_x = (uint32_t) cx;
        A.cells_y = (uint32_t) cy;
        A.n_cells = (uint32_t) (cx * cy);
        A.cell_n = (unsigned long long *) d_cell_n;
        A.cell_sum_r2 = d_cell_sum_r2;
    }
    if (d_hist) {
        A.hist_range = opt.hist_range > 0.0 ? opt.hist_range : 4.0 * s->huber_a;
        if (opt.hist_bins < 1 || opt.hist_bins > RP_MAX_HIST || !(A.hist_range > 0.0)) {
            ctx->last_error = "ecal_solver_report: 1 <= hist_bins <= 256 and a positive hist_range";
            return ECAL_ERR_INVALID;
        }
        A.hist_bins = opt.hist_bins;
        A.hist = (unsigned long long *) d_hist;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_total, 0, sizeof(ecal_report_totals), st));
    if (d_kf) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_kf, 0, (size_t) n_keyframes * sizeof(ecal_bin_stats), st));
    if (d_lm && s->n_lm) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_lm, 0, (size_t) s->n_lm * sizeof(ecal_bin_stats), st));
    if (d_cell_n) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_cell_n, 0, (size_t) A.n_cells * sizeof(uint64_t), st));
    if (d_cell_sum_r2) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_cell_sum_r2, 0, (size_t) A.n_cells * sizeof(double), st));
    if (d_hist) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t) A.hist_bins * sizeof(uint64_t), st));
    if (!s->n_chunks) return ECAL_OK;
    const size_t lds = (size_t) A.n_lm * 40 + (size_t) A.n_cells * 12 + (size_t) A.hist_bins * 4;   // <= 140 KB of the CU's 160
    if (lds > s->report_lds) {
        const void *fn = s->use_so3 ? (s->fisheye ? (const void *) &report_kernel<true, true> : (const void *) &report_kernel<true, false>)
                                    : (s->fisheye ? (const void *) &report_kernel<false, true> : (const void *) &report_kernel<false, false>);
        ECAL_HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        s->report_lds = lds;
    }
#define ECAL_RP_LAUNCH(SO3_, FISH_)                                                                                               \
    hipLaunchKernelGGL((report_kernel<SO3_, FISH_>), dim3(s->n_chunks), dim3(NE_T), lds, st, s->d_rec, s->d_chunks, s->d_knots,      \
                       s->d_knot_off, s->d_cp_off, d_params, s->n_cp, s->d_landmarks, s->radius, s->huber_a, A)
    if (s->use_so3) {
        if (s->fisheye) ECAL_RP_LAUNCH(true, true); else ECAL_RP_LAUNCH(true, false);
    } else {
        if (s->fisheye) ECAL_RP_LAUNCH(false, true); else ECAL_RP_LAUNCH(false, false);
    }
#undef ECAL_RP_LAUNCH
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_solver_report(ecal_solver *s, const double *params, const double *kf_time, uint32_t n_keyframes,
                                  const ecal_report_options *opt_in, ecal_report_totals *total, ecal_bin_stats *kf, ecal_bin_stats *lm,
                                  uint64_t *cell_n, double *cell_sum_r2, uint64_t *hist) {
    if (!s || !params || !total) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (kf && (!kf_time || n_keyframes == 0)) {
        ctx->last_error = "ecal_solver_report: per-keyframe statistics need a keyframe table";
        return ECAL_ERR_INVALID;
    }
    ecal_report_options opt;
    if (opt_in) opt = *opt_in; else ecal_report_default_options(&opt);
    if (hist && (opt.hist_bins < 1 || opt.hist_bins > RP_MAX_HIST)) {
        ctx->last_error = "ecal_solver_report: 1 <= hist_bins <= 256 and a positive hist_range";
        return ECAL_ERR_INVALID;
    }
    // the device images of the outputs, one after another in the context's scratch (sizes in 8-byte words); the _dev call
    // repeats the range checks, here the sizes only have to be safe
    const bool cells = (cell_n || cell_sum_r2) && opt.cell_px != 0;
    const uint64_t n_cells = cells ? (((uint64_t) opt.width + opt.cell_px - 1) / opt.cell_px) * (((uint64_t) opt.height + opt.cell_px - 1) / opt.cell_px) : 0;
    if (n_cells > RP_MAX_CELLS) {
        ctx->last_error = "ecal_solver_report: more than 8192 coverage cells";
        return ECAL_ERR_INVALID;
    }
    const size_t w_total = sizeof(ecal_report_totals) / 8, w_kf = kf ? 6 * (size_t) n_keyframes : 0, w_lm = lm ? 6 * (size_t) s->n_lm : 0,
                 w_cn = cell_n ? (size_t) n_cells : 0, w_cs = cell_sum_r2 ? (size_t) n_cells : 0, w_h = hist ? (size_t) opt.hist_bins : 0,
                 w_t = kf ? (size_t) n_keyframes : 0, w_out = w_total + w_kf + w_lm + w_cn + w_cs + w_h;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ecal_ensure(ctx, ctx->report_scratch, (w_out + w_t) * 8);
    if (rc) return rc;
    uint64_t *base = ctx->report_scratch.as<uint64_t>();
    uint64_t *p_total = base, *p_kf = p_total + w_total, *p_lm = p_kf + w_kf, *p_cn = p_lm + w_lm, *p_cs = p_cn + w_cn, *p_h = p_cs + w_cs,
             *p_t = p_h + w_h;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    if (w_t) ECAL_HIP_TRY(ctx, hipMemcpyAsync(p_t, kf_time, w_t * 8, hipMemcpyHostToDevice, st));
    rc = ecal_solver_report_dev(s, s->d_params, kf ? (const double *) p_t : nullptr, n_keyframes, &opt, (ecal_report_totals *) p_total,
                                kf ? (ecal_bin_stats *) p_kf : nullptr, lm ? (ecal_bin_stats *) p_lm : nullptr, cell_n ? p_cn : nullptr,
                                cell_sum_r2 ? (double *) p_cs : nullptr, hist ? p_h : nullptr, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(total, p_total, w_total * 8, hipMemcpyDeviceToHost, st));
    if (w_kf) ECAL_HIP_TRY(ctx, hipMemcpyAsync(kf, p_kf, w_kf * 8, hipMemcpyDeviceToHost, st));
    if (w_lm) ECAL_HIP_TRY(ctx, hipMemcpyAsync(lm, p_lm, w_lm * 8, hipMemcpyDeviceToHost, st));
    if (w_cn) ECAL_HIP_TRY(ctx, hipMemcpyAsync(cell_n, p_cn, w_cn * 8, hipMemcpyDeviceToHost, st));
    if (w_cs) ECAL_HIP_TRY(ctx, hipMemcpyAsync(cell_sum_r2, p_cs, w_cs * 8, hipMemcpyDeviceToHost, st));
    if (w_h) ECAL_HIP_TRY(ctx, hipMemcpyAsync(hist, p_h, w_h * 8, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}
