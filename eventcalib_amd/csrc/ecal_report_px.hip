// The calibration quality report in PIXELS (include/ecal.h, "report in pixels"; ecal_solver_report_px[_dev], ecal_residuals_px[_dev]):
// per residual record the first-order (Sampson) distance from the event to the projected rim,
//   r_px = r / |d r / d (u, v)|,
// binned per keyframe, per landmark, per sensor cell and into a histogram in one pass over the solver's records, exactly as
// ecal_report.hip bins the board-unit residual r.  d r / d (u, v) is minus the residual's analytic gradient by (cx, cy), so the
// kernel needs two numbers beside r and not the 33-column row: spline_residual_px* of spline_residual.hpp.  Why not a forward
// projection, what the definition measures and the kernels' resources: design/23_report_px.md.
//
// Floating point: r and the gradient are compiled as the solver compiles its residual (contraction to FMA allowed, the pragma
// around the include below); everything from g2 = gu * gu + gv * gv on (residual_px_distance: explicit single operations) and
// everything that decides a BIN is compiled without contraction, the file's default.
#include <hip/hip_runtime.h>
#pragma clang fp contract(fast)
#include "spline_residual.hpp"
#pragma clang fp contract(off)
#include "ecal_solver_state.hpp"
#include "block_utils.hpp"
#include "report_bins.hpp"

#include <algorithm>

namespace ecal {

struct ReportPxArgs {
    const double *kf_time;
    uint32_t n_kf, n_lm;
    uint32_t cell_px, cells_x, cells_y, n_cells;   // n_cells = 0: no coverage map
    uint32_t hist_bins;                            // 0: no histogram
    double hist_range, outlier;
    ecal_report_px_totals *total;
    ecal_bin_stats *kf, *lm;                       // NULL: family skipped
    unsigned long long *cell_n, *hist;
    double *cell_sum_r2;
};

// (the chunk's constants of both kernels, ChunkPose: ecal_solver_state.hpp)

// r and g = d r / d (u, v) of one record
template <bool SO3, bool FISHEYE>
__device__ __forceinline__ double record_residual_px(const ResRecord &e, const Chunk &ch, const ChunkPose &P, const double *landmarks,
                                                     double radius, double g[2]) {
    ResidualInput in;
    residual_input_fill(in, e, landmarks, radius, P.ifx, P.ify, P.kn, ch.span, P.binv);
    return SO3 ? spline_residual_px_so3<FISHEYE>(in, P.pin, P.q, P.t, g) : spline_residual_px<FISHEYE>(in, P.pin, P.q, P.t, g);
}

// report_kernel's shape (ecal_report.hip): one workgroup per chunk, the next record asked for before this one is evaluated, totals
// and ONE keyframe's statistics in registers (handed to the LDS bins when the keyframe changes; a chunk across more than RP_KF_LDS
// keyframes adds to global memory instead), landmark / cell / histogram bins as LDS atomics, one flush at the end.  A degenerate
// record is counted and enters no bin.
template <bool SO3, bool FISHEYE>
__global__ __launch_bounds__(NE_T) void report_px_kernel(const ResRecord *__restrict__ rec, const Chunk *__restrict__ chunks,
                                                        const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                        const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                        uint32_t n_cp_total, const double *__restrict__ landmarks, double radius,
                                                        const ReportPxArgs A) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];   // lm sums [4][n_lm] | cell sums [n_cells] | lm counts [2][n_lm] | cell counts | hist
    __shared__ double s_kt[RP_KF_LDS], s_kfsum[3 * RP_KF_LDS], s_red[5 * (NE_T / 64)];
    __shared__ unsigned long long s_kfmax[RP_KF_LDS];
    __shared__ uint32_t s_kfcnt[2 * RP_KF_LDS], s_redn[3 * (NE_T / 64)], s_bounds[2];
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
        k_first = a_lo > 0 ? a_lo - 1u : 0u;                      // the records' keyframes lie in [k_first, min(a_hi, K - 1)]
        n_bins = (a_hi < K ? a_hi : K - 1u) - k_first + 1u;
        staged = n_bins <= RP_KF_LDS;
        if (staged && (uint32_t) tid < n_bins) s_kt[tid] = A.kf_time[k_first + tid];
    }
    __syncthreads();

    ChunkPose P;
    P.load(ch, knots, knot_off, cp_off, params, n_cp_total);
    const double hist_scale_den = __dmul_rn(2.0, A.hist_range), hist_top = (double) (n_hist ? n_hist - 1u : 0u);

    BinAcc tot, cur;          // the chunk's totals; the statistics of keyframe cur_k
    uint32_t cur_k = 0, n_deg = 0;
    double sum_ppu = 0.0;     // sum of 1 / |g|: pixels per board unit
    auto kf_hand_over = [&]() {
        if (!cur.n) return;
        if (staged) kfb.add(cur_k - k_first, cur);
        else bin_add_global(A.kf + cur_k, cur);   // a chunk across more keyframes than the LDS bins hold
        cur = BinAcc();
    };

    ResRecord e_next = rec[ch.start + min((uint32_t) tid, ch.count - 1u)];
    for (uint32_t k = (uint32_t) tid; k < ch.count; k += NE_T) {
        const ResRecord e = e_next;
        e_next = rec[ch.start + min(k + (uint32_t) NE_T, ch.count - 1u)];
        double g[2], r, ppu;
        const double rb = record_residual_px<SO3, FISHEYE>(e, ch, P, landmarks, radius, g);
        if (residual_px_distance(rb, g, &r, &ppu)) {
            n_deg++;
            continue;
        }
        sum_ppu += ppu;
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
            b = b > 0.0 ? b : 0.0;
            b = b < hist_top ? b : hist_top;   // (an infinite r_px, g2 a denormal, lands in an end bin)
            atomicAdd(&hist[(uint32_t) b], 1u);
        }
    }
    kf_hand_over();

    // totals: wave reduction, then one thread adds the workgroup's five numbers and three counts
    {
        double v[5] = {tot.sum_r, tot.sum_r2, tot.sum_abs, sum_ppu, tot.max_abs};
        uint32_t c[3] = {tot.n, tot.n_out, n_deg};
        for (int o = 32; o > 0; o >>= 1) {
            for (int i = 0; i < 4; i++) v[i] += __shfl_down(v[i], o, 64);
            v[4] = fmax(v[4], __shfl_down(v[4], o, 64));
            for (int i = 0; i < 3; i++) c[i] += __shfl_down(c[i], o, 64);
        }
        if ((tid & 63) == 0) {
            for (int i = 0; i < 5; i++) s_red[5 * (tid >> 6) + i] = v[i];
            for (int i = 0; i < 3; i++) s_redn[3 * (tid >> 6) + i] = c[i];
        }
    }
    __syncthreads();   // ... and every thread's LDS bins are complete
    if (tid == 0) {
        BinAcc a;
        double ps = 0.0;
        uint32_t nd = 0;
        for (int w = 0; w < NE_T / 64; w++) {
            a.sum_r += s_red[5 * w];
            a.sum_r2 += s_red[5 * w + 1];
            a.sum_abs += s_red[5 * w + 2];
            ps += s_red[5 * w + 3];
            a.max_abs = fmax(a.max_abs, s_red[5 * w + 4]);
            a.n += s_redn[3 * w];
            a.n_out += s_redn[3 * w + 1];
            nd += s_redn[3 * w + 2];
        }
        if (a.n) {
            bin_add_global(&A.total->all, a);
            atomicAdd(&A.total->sum_px_per_unit, ps);
        }
        if (nd) atomicAdd((unsigned long long *) &A.total->n_degenerate, (unsigned long long) nd);
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

// the per-event form: r_px (0 where degenerate), optionally (gu, gv) and the verdict
template <bool SO3, bool FISHEYE>
__global__ __launch_bounds__(NE_T) void residuals_px_kernel(const ResRecord *__restrict__ rec, const Chunk *__restrict__ chunks,
                                                           const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                           const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                           uint32_t n_cp_total, const double *__restrict__ landmarks, double radius,
                                                           double *__restrict__ r_out, double *__restrict__ g_out,
                                                           uint8_t *__restrict__ flag_out) {
    const Chunk ch = chunks[blockIdx.x];
    ChunkPose P;
    P.load(ch, knots, knot_off, cp_off, params, n_cp_total);
    for (uint32_t k = threadIdx.x; k < ch.count; k += NE_T) {
        const size_t at = (size_t) ch.start + k;
        const ResRecord e = rec[at];
        double g[2], r, ppu;
        const double rb = record_residual_px<SO3, FISHEYE>(e, ch, P, landmarks, radius, g);
        const bool deg = residual_px_distance(rb, g, &r, &ppu);
        r_out[at] = r;
        if (g_out) {
            g_out[2 * at] = g[0];
            g_out[2 * at + 1] = g[1];
        }
        if (flag_out) flag_out[at] = deg ? 1 : 0;
    }
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_report_px_totals) == 64, "the pixel report's totals have no padding");

extern "C" void ecal_report_px_default_options(ecal_report_options *o) {
    if (!o) return;
    o->width = 346;   // the reference's sensor (DAVIS346)
    o->height = 260;
    o->cell_px = 16;
    o->hist_bins = 64;
    o->hist_range = 4.0;       // pixels
    o->outlier_thresh = 1.0;   // pixels
}

extern "C" int ecal_solver_report_px_dev(ecal_solver *s, const double *d_params, const double *d_kf_time, uint32_t n_keyframes,
                                         const ecal_report_options *opt_in, ecal_report_px_totals *d_total, ecal_bin_stats *d_kf,
                                         ecal_bin_stats *d_lm, uint64_t *d_cell_n, double *d_cell_sum_r2, uint64_t *d_hist,
                                         void *stream) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_report_px");
    if (!s || !d_params || !d_total) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ecal_report_options opt, def;
    ecal_report_px_default_options(&def);
    opt = opt_in ? *opt_in : def;
    ReportPxArgs A{};
    A.total = d_total;
    A.outlier = opt.outlier_thresh > 0.0 ? opt.outlier_thresh : def.outlier_thresh;
    if (d_kf) {
        if (!d_kf_time || n_keyframes == 0) {
            ctx->last_error = "ecal_solver_report_px: per-keyframe statistics need a keyframe table";
            return ECAL_ERR_INVALID;
        }
        A.kf = d_kf;
        A.kf_time = d_kf_time;
        A.n_kf = n_keyframes;
    }
    if (d_lm) {
        if (s->n_lm > RP_MAX_LM) {
            ctx->last_error = "ecal_solver_report_px: per-landmark statistics for at most 1024 landmarks";
            return ECAL_ERR_RANGE;
        }
        A.lm = d_lm;
        A.n_lm = s->n_lm;
    }
    if (d_cell_n || d_cell_sum_r2) {
        if (opt.cell_px == 0 || opt.width == 0 || opt.height == 0) {
            ctx->last_error = "ecal_solver_report_px: the coverage map needs width, height and cell_px > 0";
            return ECAL_ERR_INVALID;
        }
        const uint64_t cx = ((uint64_t) opt.width + opt.cell_px - 1) / opt.cell_px, cy = ((uint64_t) opt.height + opt.cell_px - 1) / opt.cell_px;
        if (cx * cy > RP_MAX_CELLS) {
            ctx->last_error = "ecal_solver_report_px: more than 8192 coverage cells";
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
        A.hist_range = opt.hist_range > 0.0 ? opt.hist_range : def.hist_range;
        if (opt.hist_bins < 1 || opt.hist_bins > RP_MAX_HIST || !(A.hist_range > 0.0)) {
            ctx->last_error = "ecal_solver_report_px: 1 <= hist_bins <= 256 and a positive hist_range";
            return ECAL_ERR_INVALID;
        }
        A.hist_bins = opt.hist_bins;
        A.hist = (unsigned long long *) d_hist;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_total, 0, sizeof(ecal_report_px_totals), st));
    if (d_kf) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_kf, 0, (size_t) n_keyframes * sizeof(ecal_bin_stats), st));
    if (d_lm && s->n_lm) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_lm, 0, (size_t) s->n_lm * sizeof(ecal_bin_stats), st));
    if (d_cell_n) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_cell_n, 0, (size_t) A.n_cells * sizeof(uint64_t), st));
    if (d_cell_sum_r2) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_cell_sum_r2, 0, (size_t) A.n_cells * sizeof(double), st));
    if (d_hist) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t) A.hist_bins * sizeof(uint64_t), st));
    if (!s->n_chunks) return ECAL_OK;
    const size_t lds = (size_t) A.n_lm * 40 + (size_t) A.n_cells * 12 + (size_t) A.hist_bins * 4;   // <= 140 KB of the CU's 160
    if (lds > s->report_px_lds) {
        const void *fn = s->use_so3 ? (s->fisheye ? (const void *) &report_px_kernel<true, true> : (const void *) &report_px_kernel<true, false>)
                                    : (s->fisheye ? (const void *) &report_px_kernel<false, true> : (const void *) &report_px_kernel<false, false>);
        ECAL_HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        s->report_px_lds = lds;
    }
#define ECAL_RPX_LAUNCH(SO3_, FISH_)                                                                                                \
    hipLaunchKernelGGL((report_px_kernel<SO3_, FISH_>), dim3(s->n_chunks), dim3(NE_T), lds, st, s->d_rec, s->d_chunks, s->d_knots,   \
                       s->d_knot_off, s->d_cp_off, d_params, s->n_cp, s->d_landmarks, s->radius, A)
    if (s->use_so3) {
        if (s->fisheye) ECAL_RPX_LAUNCH(true, true); else ECAL_RPX_LAUNCH(true, false);
    } else {
        if (s->fisheye) ECAL_RPX_LAUNCH(false, true); else ECAL_RPX_LAUNCH(false, false);
    }
#undef ECAL_RPX_LAUNCH
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_solver_report_px(ecal_solver *s, const double *params, const double *kf_time, uint32_t n_keyframes,
                                     const ecal_report_options *opt_in, ecal_report_px_totals *total, ecal_bin_stats *kf,
                                     ecal_bin_stats *lm, uint64_t *cell_n, double *cell_sum_r2, uint64_t *hist) {
    if (!s || !params || !total) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (kf && (!kf_time || n_keyframes == 0)) {
        ctx->last_error = "ecal_solver_report_px: per-keyframe statistics need a keyframe table";
        return ECAL_ERR_INVALID;
    }
    ecal_report_options opt;
    if (opt_in) opt = *opt_in; else ecal_report_px_default_options(&opt);
    if (hist && (opt.hist_bins < 1 || opt.hist_bins > RP_MAX_HIST)) {
        ctx->last_error = "ecal_solver_report_px: 1 <= hist_bins <= 256 and a positive hist_range";
        return ECAL_ERR_INVALID;
    }
    // the device images of the outputs, one after another in the context's scratch (sizes in 8-byte words), as ecal_solver_report
    // lays them out; the _dev call repeats the range checks, here the sizes only have to be safe
    const bool cells = (cell_n || cell_sum_r2) && opt.cell_px != 0;
    const uint64_t n_cells = cells ? (((uint64_t) opt.width + opt.cell_px - 1) / opt.cell_px) * (((uint64_t) opt.height + opt.cell_px - 1) / opt.cell_px) : 0;
    if (n_cells > RP_MAX_CELLS) {
        ctx->last_error = "ecal_solver_report_px: more than 8192 coverage cells";
        return ECAL_ERR_INVALID;
    }
    const size_t w_total = sizeof(ecal_report_px_totals) / 8, w_kf = kf ? 6 * (size_t) n_keyframes : 0, w_lm = lm ? 6 * (size_t) s->n_lm : 0,
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
    rc = ecal_solver_report_px_dev(s, s->d_params, kf ? (const double *) p_t : nullptr, n_keyframes, &opt, (ecal_report_px_totals *) p_total,
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

extern "C" int ecal_residuals_px_dev(ecal_solver *s, const double *d_params, double *d_r_px, double *d_grad, uint8_t *d_flag,
                                     void *stream) {
    if (!s || !d_params || (s->n_res && !d_r_px)) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    if (s->n_chunks) {
#define ECAL_RPX_LAUNCH(SO3_, FISH_)                                                                                                 \
    hipLaunchKernelGGL((residuals_px_kernel<SO3_, FISH_>), dim3(s->n_chunks), dim3(NE_T), 0, st, s->d_rec, s->d_chunks, s->d_knots,  \
                       s->d_knot_off, s->d_cp_off, d_params, s->n_cp, s->d_landmarks, s->radius, d_r_px, d_grad, d_flag)
        if (s->use_so3) {
            if (s->fisheye) ECAL_RPX_LAUNCH(true, true); else ECAL_RPX_LAUNCH(true, false);
        } else {
            if (s->fisheye) ECAL_RPX_LAUNCH(false, true); else ECAL_RPX_LAUNCH(false, false);
        }
#undef ECAL_RPX_LAUNCH
        ECAL_HIP_TRY(ctx, hipGetLastError());
    }
    return ECAL_OK;
}

extern "C" int ecal_residuals_px(ecal_solver *s, const double *params, double *r_px, double *grad, uint8_t *flag) {
    if (!s || !params || (s->n_res && !r_px)) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = s->n_res;
    if (!n) return ECAL_OK;
    // r_px [n] | grad [n][2] | flag [n] in the context's report scratch
    const size_t w_r = n, w_g = grad ? 2 * n : 0, w_f = flag ? (n + 7) / 8 : 0;
    int rc = ecal_ensure(ctx, ctx->report_scratch, (w_r + w_g + w_f) * 8);
    if (rc) return rc;
    double *d_r = ctx->report_scratch.as<double>(), *d_g = grad ? d_r + w_r : nullptr;
    uint8_t *d_f = flag ? reinterpret_cast<uint8_t *>(d_r + w_r + w_g) : nullptr;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    rc = ecal_residuals_px_dev(s, s->d_params, d_r, d_g, d_f, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(r_px, d_r, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (grad) ECAL_HIP_TRY(ctx, hipMemcpyAsync(grad, d_g, 2 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (flag) ECAL_HIP_TRY(ctx, hipMemcpyAsync(flag, d_f, n, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}
