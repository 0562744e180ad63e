// Uncertainty of the intrinsics, the device half (include/ecal_uncertainty.h; design/24_uncertainty.md):
//   chunk_score_kernel   per chunk of the solver's records the sum of rho' r J (33 columns) and of rho / 2: the gradient of the robust
//                        cost split by chunk, which the cluster-robust covariance is built from (ecal_solver_uncertainty,
//                        ecal_solver.hip + arrow_covariance.hpp).  The residual-and-Jacobian code of normal_eq_kernel without the Gram
//                        matrix: no LDS rows, no matrix cores, no atomics; the workgroup's sum is taken in a fixed order.
//   sigma_map_kernel     one thread a pixel: uncertainty_point.hpp, shared with ecal_uncertainty_map_host.
//
// Floating point: r, the row and the loss are compiled as the solver compiles them (contraction to FMA allowed, the pragma around
// the include below, as in ecal_report_px.hip); the accumulation is an explicit fma per column (the matrix cores of
// normal_eq_kernel fuse the same product into their sum); the sigma map is compiled without contraction, the file's default.
#include <hip/hip_runtime.h>
#pragma clang fp contract(fast)
#include "spline_residual.hpp"
#pragma clang fp contract(off)
#include "ecal_solver_state.hpp"
#include "uncertainty_point.hpp"
#include "../../include/ecal_uncertainty.h"

#include <vector>

namespace ecal {

constexpr int CS_N = RES_NJ + 1;   // 33 score columns and rho / 2

// One workgroup per chunk (report_px_kernel's shape: the next record is asked for before this one is evaluated).  A thread adds
// its records k = tid, tid + NE_T, .. in that order into 34 private sums; the waves reduce by shuffles (a fixed tree), the four
// waves' sums go through LDS and are added wave 0 first.  Nothing depends on the order in which workgroups or waves run.
template <bool SO3, bool FISHEYE>
__global__ __launch_bounds__(NE_T) void chunk_score_kernel(const ResRecord *__restrict__ rec, const Chunk *__restrict__ chunks,
                                                          const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                          const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                          uint32_t n_cp_total, const double *__restrict__ landmarks, double radius,
                                                          double huber_a, double *__restrict__ score_out,
                                                          double *__restrict__ half_rho_out) {
    __shared__ double s_red[(NE_T / 64) * CS_N];
    const Chunk ch = chunks[blockIdx.x];
    const int tid = threadIdx.x;
    ChunkPose P;
    P.load(ch, knots, knot_off, cp_off, params, n_cp_total);
    const double inv_huber_a = 1.0 / huber_a;

    double acc[CS_N];
#pragma unroll
    for (int i = 0; i < CS_N; i++) acc[i] = 0.0;

    ResRecord e_next = rec[ch.start + min((uint32_t) tid, ch.count - 1u)];
    for (uint32_t k = (uint32_t) tid; k < ch.count; k += NE_T) {
        const ResRecord e = e_next;
        e_next = rec[ch.start + min(k + (uint32_t) NE_T, ch.count - 1u)];
        ResidualInput in;
        residual_input_fill(in, e, landmarks, radius, P.ifx, P.ify, P.kn, ch.span, P.binv);
        double sc = 0.0, hr = 0.0, J[RES_NJ];
        in.huber_a = huber_a;      // the core applies the loss: the row comes out scaled by sqrt(rho') (ResidualInput)
        in.inv_huber_a = inv_huber_a;
        in.sc_out = &sc;
        in.half_rho_out = &hr;
        const double r = SO3 ? spline_residual_so3<FISHEYE>(in, P.pin, P.q, P.t, J) : spline_residual<FISHEYE>(in, P.pin, P.q, P.t, J);
        const double rt = __dmul_rn(r, sc);   // normal_eq_kernel's column 33
#pragma unroll
        for (int i = 0; i < RES_NJ; i++) acc[i] = fma(rt, J[i], acc[i]);
        acc[RES_NJ] = __dadd_rn(acc[RES_NJ], hr);
    }

#pragma unroll
    for (int i = 0; i < CS_N; i++) {
        double v = acc[i];
        for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_down(v, o, 64));
        if ((tid & 63) == 0) s_red[(tid >> 6) * CS_N + i] = v;
    }
    __syncthreads();
    if (tid < CS_N) {
        double v = s_red[tid];
        for (int w = 1; w < NE_T / 64; w++) v = __dadd_rn(v, s_red[w * CS_N + tid]);
        if (tid < RES_NJ) score_out[(size_t) blockIdx.x * RES_NJ + tid] = v;
        else if (half_rho_out) half_rho_out[blockIdx.x] = v;
    }
}

struct SigmaMapArgs {
    double intr[9], cov[81];
    int model;
    uint32_t width, height;
};

__global__ __launch_bounds__(256) void sigma_map_kernel(const SigmaMapArgs A, double *__restrict__ sigma, uint8_t *__restrict__ flag) {
    const size_t n = (size_t) A.width * A.height, i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = (uint32_t) (i / A.width), col = (uint32_t) (i - (size_t) row * A.width);
    double s;
    const uint8_t f = ecal_uncertainty::uq_pixel(A.model, A.intr, A.cov, (double) col, (double) row, &s, nullptr);
    sigma[i] = s;
    if (flag) flag[i] = f;
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_uncertainty_result) == 8 + 4 * 4 + 4 * 4 + 2 * 8 + (81 + 9 + 81 + 81 + 9 + 9) * 8, "the result has no padding");

extern "C" int ecal_solver_chunk_scores_dev(ecal_solver *s, const double *d_params, double *d_score, double *d_half_rho, void *stream) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_chunk_scores");
    if (!s || !d_params || (s->n_chunks && !d_score)) return ECAL_ERR_INVALID;
    if (!s->n_chunks) return ECAL_OK;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
#define ECAL_CS_LAUNCH(SO3_, FISH_)                                                                                                 \
    hipLaunchKernelGGL((chunk_score_kernel<SO3_, FISH_>), dim3(s->n_chunks), dim3(NE_T), 0, st, s->d_rec, s->d_chunks, s->d_knots,  \
                       s->d_knot_off, s->d_cp_off, d_params, s->n_cp, s->d_landmarks, s->radius, s->huber_a, d_score, d_half_rho)
    if (s->use_so3) {
        if (s->fisheye) ECAL_CS_LAUNCH(true, true); else ECAL_CS_LAUNCH(true, false);
    } else {
        if (s->fisheye) ECAL_CS_LAUNCH(false, true); else ECAL_CS_LAUNCH(false, false);
    }
#undef ECAL_CS_LAUNCH
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_solver_chunk_scores(ecal_solver *s, const double *params, double *score, double *half_rho) {
    if (!s || !params || (s->n_chunks && !score)) return ECAL_ERR_INVALID;
    if (!s->n_chunks) return ECAL_OK;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = s->n_chunks;
    int rc = ecal_ensure(ctx, ctx->report_scratch, n * CS_N * sizeof(double));   // score [n][33] | half_rho [n]
    if (rc) return rc;
    double *d_score = ctx->report_scratch.as<double>(), *d_hr = d_score + n * RES_NJ;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    rc = ecal_solver_chunk_scores_dev(s, s->d_params, d_score, d_hr, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(score, d_score, n * RES_NJ * sizeof(double), hipMemcpyDeviceToHost, st));
    if (half_rho) ECAL_HIP_TRY(ctx, hipMemcpyAsync(half_rho, d_hr, n * sizeof(double), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}

extern "C" int ecal_solver_chunk_table(ecal_solver *s, uint32_t *out) {
    if (!s || (s->n_chunks && !out)) return ECAL_ERR_INVALID;
    if (!s->n_chunks) return ECAL_OK;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<Chunk> h(s->n_chunks);
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(h.data(), s->d_chunks, h.size() * sizeof(Chunk), hipMemcpyDeviceToHost, ctx->stream));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < h.size(); c++) {
        if (h[c].seg >= s->n_seg) {
            ctx->last_error = "ecal_solver_chunk_table: a chunk names a segment the solver does not have";
            return ECAL_ERR_RANGE;
        }
        out[4 * c] = s->cp_off[h[c].seg] + h[c].span - 3;
        out[4 * c + 1] = h[c].count;
        out[4 * c + 2] = h[c].seg;
        out[4 * c + 3] = h[c].span;
    }
    return ECAL_OK;
}

extern "C" void ecal_uncertainty_default_options(ecal_uncertainty_options *o) {
    if (!o) return;
    o->cluster_spans = 1;
    o->reserved = 0;
}

static bool sigma_map_args(int camera_model, const double *intr9, const double *cov81, uint32_t width, uint32_t height, SigmaMapArgs &A) {
    if (!intr9 || !cov81 || (camera_model != ECAL_CAMERA_RADIAL && camera_model != ECAL_CAMERA_FISHEYE)) return false;
    if (width < 1 || width > 8192 || height < 1 || height > 8192) return false;
    using ecal_undistort::ud_finite;
    if (!(ud_finite(intr9[0]) && intr9[0] > 0.0 && ud_finite(intr9[1]) && intr9[1] > 0.0)) return false;
    for (int i = 0; i < 9; i++) A.intr[i] = intr9[i];
    for (int i = 0; i < 81; i++) A.cov[i] = cov81[i];
    A.model = camera_model;
    A.width = width;
    A.height = height;
    return true;
}

extern "C" int ecal_uncertainty_map_host(int camera_model, const double *intr9, const double *cov81, uint32_t width, uint32_t height,
                                         double *sigma_px, uint8_t *flag, double *jac) {
    SigmaMapArgs A;
    if (!sigma_px || !sigma_map_args(camera_model, intr9, cov81, width, height, A)) return ECAL_ERR_INVALID;
    for (uint32_t row = 0; row < height; row++)
        for (uint32_t col = 0; col < width; col++) {
            const size_t i = (size_t) row * width + col;
            const uint8_t f = ecal_uncertainty::uq_pixel(A.model, A.intr, A.cov, (double) col, (double) row, &sigma_px[i], jac ? jac + 18 * i : nullptr);
            if (flag) flag[i] = f;
        }
    return ECAL_OK;
}

extern "C" int ecal_uncertainty_map_dev(ecal_ctx *ctx, int camera_model, const double *intr9, const double *cov81, uint32_t width,
                                        uint32_t height, double *d_sigma_px, uint8_t *d_flag, void *stream) {
    if (!ctx) return ECAL_ERR_INVALID;
    SigmaMapArgs A;
    if (!d_sigma_px || !sigma_map_args(camera_model, intr9, cov81, width, height, A)) {
        ctx->last_error = "ecal_uncertainty_map: a camera model of ecal.h, fx and fy finite and above 0, width and height from 1 to 8192";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t) width * height;
    hipLaunchKernelGGL(sigma_map_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, A, d_sigma_px, d_flag);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}
