// Re-association through the solved spline (include/ecal.h, ecal_solver_reassociate[_dev] / ecal_solver_create_reassociated):
// every raw event of the stream carried through the intrinsics and the spline pose of the CURRENT parameters onto the board, and
// kept as a residual of the nearest circle when its board point lies within ring_tol of that circle's rim — wherever the event
// sits relative to a keyframe.  The keyframe association (ecal_associate.hip, EventCalibSpline.cpp:140-192) chooses the data term
// once, before the solve; the reference's own TODO there names this step ("after that re-explore the raw measurements").  New
// functionality; opt-in everywhere it is wired (calibrate_stream(refine_rounds=...), the driver's RefineRounds key).
//
// Rank-local and single-process: the multi-GPU paths (time shards, per-rank segments) do not call it.
//
// Three launches over the packed 25-byte records, blocks of ECAL_BOARD_IMAGE_BLOCK events per workgroup, and NO waiting between
// workgroups (no look-back, no flag anybody spins on):
//   1. reassoc_verdict_kernel  the board image's per-event arithmetic (board_block.hpp: the block's plan, the pose fetch;
//                              spline_residual.hpp: pose and board point; board_nearest.hpp: nearest landmark, d, the gate), ONE
//                              verdict byte per event — the landmark index, or 0xFF for "not kept" — and one count per block
//   2. the exclusive scan of the blocks' counts by one workgroup (ecal_scan_blocks, the association's)
//   3. reassoc_write_kernel    reads the verdicts (16 bytes per thread), scans inside the block in event order and copies the kept
//                              events' own bytes into obs / time, with lm_id and seg_id
// so the pose arithmetic runs once per event.  Bytes per event: 25 read + 1 written in pass 1; 1 read in pass 2, and per KEPT
// event 24 read + 32 written.  Design and LDS budget: design/08_solver.md, "Re-association".
//
// Floating point: the board point is compiled as the solver compiles its residual (contraction to FMA allowed, the pragma around
// the include); everything that decides (nearest landmark, d, the gate) is compiled without contraction, the file's default.
#include <hip/hip_runtime.h>
#pragma clang fp contract(fast)
#include "spline_residual.hpp"
#pragma clang fp contract(off)
#include "ecal_solver_state.hpp"
#include "stream_compact.hpp"
#include "board_nearest.hpp"
#include "board_block.hpp"

#include <cmath>

namespace ecal {

constexpr uint32_t RA_NTOT = 5;    // words of ecal_reassociate_totals
static_assert(BI_BLOCK == SC_BLOCK && BI_T == SC_T, "the writing pass reads its verdicts as the stream filters do (stream_compact.hpp)");

template <bool SO3, bool FISHEYE>
__global__ __launch_bounds__(BI_T, 2) void reassoc_verdict_kernel(const uint8_t *__restrict__ rec, uint64_t n_events,
                                                              const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                              const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                              const double *__restrict__ seg_range, uint32_t n_seg, uint32_t n_cp_total,
                                                              const double *__restrict__ landmarks, uint32_t n_lm, double radius,
                                                              double ring_tol, uint8_t *__restrict__ verdict,
                                                              uint32_t *__restrict__ block_cnt, unsigned long long *__restrict__ totals) {
    const BoardSpline S{knots, knot_off, cp_off, params, seg_range, n_seg, n_cp_total};   // (built here: the arguments keep their __restrict__)
    __shared__ BoardBlockLds s_blk;
    __shared__ double s_lm[2 * BI_MAX_LM];
    __shared__ uint32_t s_red[(BI_T / 64) * RA_NTOT];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * BI_BLOCK;
    const uint32_t count = stream_block_count(n_events, base);
    const uint8_t *const blk = rec + base * 25;
    for (uint32_t i = (uint32_t) tid; i < n_lm; i += BI_T) {   // (n_lm <= BI_MAX_LM: the entry point checks)
        s_lm[2 * i] = landmarks[3 * (size_t) i];
        s_lm[2 * i + 1] = landmarks[3 * (size_t) i + 1];
    }
    const BoardBlockPlan P = board_block_plan(blk, count, S, s_blk);   // (its barriers also publish the landmarks)

    double pin[9];
    for (int i = 0; i < 9; i++) pin[i] = S.params[i];
    const double ifx = 1.0 / pin[0], ify = 1.0 / pin[1];
    uint32_t tot[RA_NTOT] = {0, 0, 0, 0, 0};   // n_events, n_outside_time, n_behind, n_off_ring, n_kept

    for (uint32_t k = (uint32_t) tid; k < count; k += BI_T) {
        const uint8_t *r = blk + (size_t) k * 25;
        const double et = bi_load_f64(r), eu = bi_load_f64(r + 8), ev = bi_load_f64(r + 16);
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
        uint32_t v = BOARD_NOT_KEPT;
        if (!in_time) {
            tot[1]++;
        } else if (!ok) {
            tot[2]++;
        } else {
            double d;
            v = board_ring_gate(s_lm, n_lm, Xw[0], Xw[1], radius, ring_tol, &d);
            tot[v == BOARD_NOT_KEPT ? 3 : 4]++;
        }
        verdict[base + k] = (uint8_t) v;
    }

    // totals: per wave, then the block's count of kept events and one atomic per workgroup and field
    for (int o = 32; o > 0; o >>= 1)
        for (uint32_t i = 0; i < RA_NTOT; i++) tot[i] += __shfl_down(tot[i], o, 64);
    if ((tid & 63) == 0)
        for (uint32_t i = 0; i < RA_NTOT; i++) s_red[(tid >> 6) * RA_NTOT + i] = tot[i];
    __syncthreads();
    if ((uint32_t) tid < RA_NTOT) {
        uint32_t v = 0;
        for (int w = 0; w < BI_T / 64; w++) v += s_red[w * RA_NTOT + tid];
        if (tid == 4) block_cnt[blockIdx.x] = v;
        if (totals && v) atomicAdd(&totals[tid], (unsigned long long) v);
    }
}

// verdict: rounded up to whole blocks (the bytes behind n_events are read and masked, never written)
__global__ __launch_bounds__(BI_T) void reassoc_write_kernel(const uint8_t *__restrict__ rec, uint64_t n_events,
                                                            const uint8_t *__restrict__ verdict, const uint32_t *__restrict__ block_off,
                                                            const double *__restrict__ seg_range, uint32_t n_seg,
                                                            double *__restrict__ obs, double *__restrict__ time,
                                                            uint32_t *__restrict__ lm, uint32_t *__restrict__ seg) {
    __shared__ double s_seg[2 * BI_SEG_LDS];
    __shared__ uint32_t s_wsum[BI_T / 64];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t) blockIdx.x * BI_BLOCK;
    const uint32_t count = stream_block_count(n_events, base);
    const bool seg_lds = n_seg <= BI_SEG_LDS;
    if (seg_lds && (uint32_t) tid < 2 * n_seg) s_seg[tid] = seg_range[tid];
    const uint32_t k0 = (uint32_t) tid * SC_PER;
    uint4 w;
    const uint32_t bits = verdict_keep_bits<BOARD_NOT_KEPT>(verdict, base, k0, count, &w);
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    // the kept events in front of this thread's (thread order = event order; the barrier inside also publishes s_seg)
    uint64_t at = (uint64_t) block_off[blockIdx.x] + block_exscan_u32<BI_T>((uint32_t) __popc(bits), s_wsum);
    if (!bits) return;
#pragma unroll
    for (uint32_t e = 0; e < SC_PER; e++) {
        if (bits >> e & 1u) {
            const uint8_t *r = rec + (base + k0 + e) * 25;
            const double et = bi_load_f64(r);
            obs[2 * at] = bi_load_f64(r + 8);
            obs[2 * at + 1] = bi_load_f64(r + 16);
            time[at] = et;
            lm[at] = (words[e >> 2] >> (8u * (e & 3u))) & 0xFFu;
            seg[at] = (uint32_t) bi_segment_of(et, seg_lds ? s_seg : seg_range, n_seg);   // (kept: the time lies in a segment)
            at++;
        }
    }
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_reassociate_totals) == 8 * RA_NTOT, "ecal_reassociate_totals has no padding");

// the tolerance in force: <= 0 means the solver's huber_a (the convention of ecal_report_options.outlier_thresh)
static int reassoc_tol(ecal_solver *s, double ring_tol, double *tol) {
    if (!std::isfinite(ring_tol)) {
        s->ctx->last_error = "ecal_solver_reassociate: a finite ring_tol (<= 0: the solver's huber_a)";
        return ECAL_ERR_INVALID;
    }
    *tol = ring_tol > 0.0 ? ring_tol : s->huber_a;
    if (s->n_lm > BI_MAX_LM) {
        s->ctx->last_error = "ecal_solver_reassociate: the re-association takes at most 128 landmarks";
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

extern "C" int ecal_solver_reassociate_dev(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events,
                                           double ring_tol, double *d_obs, double *d_time, uint32_t *d_lm_id, uint32_t *d_seg_id,
                                           uint32_t *d_count, ecal_reassociate_totals *d_totals, void *stream) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_reassociate");
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!d_params || !d_count || (n_events && (!d_events || !d_obs || !d_time || !d_lm_id || !d_seg_id))) {
        ctx->last_error = "ecal_solver_reassociate: null pointer (parameters, count, events or outputs)";
        return ECAL_ERR_INVALID;
    }
    int rc = ecal_events_range_check(ctx, "ecal_solver_reassociate", n_events);
    if (rc) return rc;
    double tol;
    if ((rc = reassoc_tol(s, ring_tol, &tol))) return rc;
    hipStream_t st = (hipStream_t) stream;
    if ((rc = ecal_compact_begin(ctx, "ecal_solver_reassociate", d_events, n_events, nullptr, d_count, d_totals, sizeof(ecal_reassociate_totals), st)))
        return rc;
    if (!n_events) return ECAL_OK;
    ecal_verdict_tables V;
    if ((rc = ecal_verdict_tables_ensure(ctx, ctx->reassoc_scratch, n_events, &V))) return rc;
    unsigned long long *tot = (unsigned long long *) d_totals;
#define ECAL_RA_LAUNCH(SO3_, FISH_)                                                                                                      \
    hipLaunchKernelGGL((reassoc_verdict_kernel<SO3_, FISH_>), dim3(V.nb), dim3(BI_T), 0, st, d_events, n_events,                          \
                       (const double *) s->d_knots, (const uint32_t *) s->d_knot_off, (const uint32_t *) s->d_cp_off, d_params,           \
                       (const double *) s->d_seg_range, s->n_seg, s->n_cp, (const double *) s->d_landmarks, s->n_lm, s->radius, tol, V.verdict, V.cnt, tot)
    if (s->use_so3) {
        if (s->fisheye) ECAL_RA_LAUNCH(true, true); else ECAL_RA_LAUNCH(true, false);
    } else {
        if (s->fisheye) ECAL_RA_LAUNCH(false, true); else ECAL_RA_LAUNCH(false, false);
    }
#undef ECAL_RA_LAUNCH
    return ecal_compact_by_verdict(ctx, V, d_count, nullptr, st, [&]() {
        hipLaunchKernelGGL(reassoc_write_kernel, dim3(V.nb), dim3(BI_T), 0, st, d_events, n_events, (const uint8_t *) V.verdict,
                           (const uint32_t *) V.off, (const double *) s->d_seg_range, s->n_seg, d_obs, d_time, d_lm_id, d_seg_id);
    });
}

namespace {
// the record arrays of the host forms in the context's scratch: obs 16 + time 8 + lm_id 4 + seg_id 4 bytes per event, then the
// count and the totals (with the verdict byte of the _dev form's own scratch: 33 bytes per event plus the block tables)
struct ReassocRecords {
    double *obs, *time;
    uint32_t *lm, *seg, *count;
    ecal_reassociate_totals *totals;
};
int reassoc_records(ecal_ctx *ctx, uint64_t n, ReassocRecords *R) {
    const size_t o_tm = (size_t) n * 16, o_lm = o_tm + (size_t) n * 8, o_sg = o_lm + (size_t) n * 4, o_tot = (o_sg + (size_t) n * 4 + 7) / 8 * 8,
                 o_cnt = o_tot + sizeof(ecal_reassociate_totals);
    const int rc = ecal_ensure(ctx, ctx->reassoc_records, o_cnt + 8);
    if (rc) return rc;
    char *base = ctx->reassoc_records.as<char>();
    R->obs = (double *) base;
    R->time = (double *) (base + o_tm);
    R->lm = (uint32_t *) (base + o_lm);
    R->seg = (uint32_t *) (base + o_sg);
    R->totals = (ecal_reassociate_totals *) (base + o_tot);
    R->count = (uint32_t *) (base + o_cnt);
    return ECAL_OK;
}
// the pass on the context's stream into the context's scratch; the count and the totals come back (one small read)
int reassoc_into_scratch(ecal_solver *s, const double *params, const ecal_stream *es, double ring_tol, ReassocRecords *R, uint32_t *count,
                         ecal_reassociate_totals *totals) {
    ecal_ctx *ctx = s->ctx;
    const uint64_t n = ecal_stream_size(es);
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = reassoc_records(ctx, n, R);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    rc = ecal_solver_reassociate_dev(s, s->d_params, ecal_stream_data(es), n, ring_tol, R->obs, R->time, R->lm, R->seg, R->count, R->totals, st);
    if (rc) return rc;
    ecal_reassociate_totals tot;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(&tot, R->totals, sizeof(tot), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(count, R->count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (totals) *totals = tot;
    return ECAL_OK;
}
}  // namespace

extern "C" int ecal_solver_reassociate(ecal_solver *s, const double *params, const ecal_stream *es, double ring_tol, uint64_t capacity,
                                       double *obs, double *time, uint32_t *lm_id, uint32_t *seg_id, uint64_t *count,
                                       ecal_reassociate_totals *totals) {
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!params || !es || !count) {
        ctx->last_error = "ecal_solver_reassociate: null pointer (parameters, stream or count)";
        return ECAL_ERR_INVALID;
    }
    *count = 0;
    ReassocRecords R;
    uint32_t cnt = 0;
    int rc = reassoc_into_scratch(s, params, es, ring_tol, &R, &cnt, totals);
    if (rc) return rc;
    *count = cnt;
    if (cnt > capacity) {
        ctx->last_error = "ecal_solver_reassociate: more records than the capacity";
        return ECAL_ERR_RANGE;
    }
    if (cnt) {
        if (!obs || !time || !lm_id || !seg_id) {
            ctx->last_error = "ecal_solver_reassociate: null pointer (outputs)";
            return ECAL_ERR_INVALID;
        }
        hipStream_t st = ctx->stream;
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(obs, R.obs, (size_t) cnt * 16, hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(time, R.time, (size_t) cnt * 8, hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(lm_id, R.lm, (size_t) cnt * 4, hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipMemcpyAsync(seg_id, R.seg, (size_t) cnt * 4, hipMemcpyDeviceToHost, st));
        ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return ECAL_OK;
}

extern "C" int ecal_solver_create_reassociated(ecal_solver *s, const double *params, const ecal_stream *es, double ring_tol,
                                               ecal_solver **out, ecal_reassociate_totals *totals) {
    if (!s) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    if (!params || !es || !out) {
        ctx->last_error = "ecal_solver_reassociate: null pointer (parameters, stream or the new solver)";
        return ECAL_ERR_INVALID;
    }
    *out = nullptr;
    ReassocRecords R;
    uint32_t cnt = 0;
    const int rc = reassoc_into_scratch(s, params, es, ring_tol, &R, &cnt, totals);
    if (rc) return rc;
    // the layout of s from its host copies, the records where the pass left them: nothing proportional to the events crosses PCIe
    ecal_spline_problem p{};
    p.n_segments = s->n_seg;
    p.seg_cp_off = s->cp_off.data();
    p.knots = s->knots.data();
    p.n_res = cnt;
    p.obs = R.obs;
    p.time = R.time;
    p.lm_id = R.lm;
    p.seg_id = R.seg;
    p.n_landmarks = s->n_lm;
    p.landmarks = s->landmarks.data();
    p.circle_radius = s->radius;
    p.huber_a = s->huber_a;
    p.use_so3 = s->use_so3 ? 1 : 0;
    p.camera_model = s->fisheye ? ECAL_CAMERA_FISHEYE : ECAL_CAMERA_RADIAL;
    return ecal_solver_create_dev(ctx, &p, nullptr, ctx->stream, out);
}
