// The block plan of the passes that carry every event of a packed, time-sorted stream through the solver's spline
// (ecal_board_image.hip, ecal_reassociate.hip): a block of ECAL_BOARD_IMAGE_BLOCK consecutive events per workgroup meets a handful
// of consecutive knot spans of one segment, so its first and last span are found once per workgroup (waves 0 and 1) and their
// control points and knots are staged in LDS; a block that meets more than ECAL_BOARD_IMAGE_CP_LDS control points or more than one
// segment reads them from global memory per event instead.  Same decisions either way (include/ecal.h, "Board-frame event image").
//
// Include AFTER spline_residual.hpp (spline_find_span, spline_basis: compiled as the solver compiles them) and with
// `fp contract(off)` in force; nothing here rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ecal.h"

namespace ecal {

constexpr int BI_T = 256;
constexpr uint32_t BI_BLOCK = ECAL_BOARD_IMAGE_BLOCK, BI_CP = ECAL_BOARD_IMAGE_CP_LDS, BI_KN = BI_CP + 4;
constexpr uint32_t BI_MAX_LM = 128, BI_SEG_LDS = 32;

__device__ __forceinline__ double bi_load_f64(const uint8_t *p) {
    double v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// the number of leading elements of the ascending p[0], p[stride], .. (K of them) that are < t (LE: <= t), by one wave: a 64-ary
// search as wave_lower_bound (block_utils.hpp).  Every lane of the wave calls it with the same arguments.
template <bool LE>
__device__ __forceinline__ uint32_t bi_wave_count(const double *p, uint32_t stride, uint32_t K, double t) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = K;
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint32_t idx = lo + lane * step;
        bool less = false;
        if (idx < hi) {
            const double x = p[(size_t) idx * stride];
            less = LE ? x <= t : x < t;
        }
        const uint32_t c = (uint32_t) __popcll(__ballot(less));
        if (c == 0) {
            hi = lo;
        } else {
            const uint32_t nhi = lo + c * step < hi ? lo + c * step : hi;
            lo = lo + (c - 1u) * step + 1u;
            hi = nhi;
        }
    }
    return lo;
}

// the segment g with range[2 g] <= t <= range[2 g + 1], or -1 (also for a NaN).  The ranges are ascending and disjoint (what
// ecal_solver_create_from_stream checks); where two of them touch at one time, that time belongs to the EARLIER one: here, in the
// block's plan below (the first segment whose end is not below the time) and in include/ecal.h.
__device__ __forceinline__ int bi_segment_of(double t, const double *range, uint32_t n_seg) {
    uint32_t a = 0, b = n_seg;   // first segment whose end is not below t
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (range[2 * m + 1] < t) a = m + 1; else b = m;
    }
    return (a < n_seg && t >= range[2 * a]) ? (int) a : -1;
}

enum { BI_NONE = 0, BI_STAGED = 1, BI_GLOBAL = 2 };

// the spline as the kernels see it (built INSIDE the kernel from its __restrict__ arguments: passed as one by-value argument the
// pointers lose that, the uniform loads behind them turn from scalar into vector loads and the kernels lose a wave per SIMD)
struct BoardSpline {
    const double *knots;
    const uint32_t *knot_off, *cp_off;
    const double *params;      // [ 9 intrinsics | q [n_cp_total][4] | t [n_cp_total][3] ]
    const double *seg_range;   // [n_seg][2]
    uint32_t n_seg, n_cp_total;
};

// the workgroup's LDS of the plan (one object, __shared__)
struct BoardBlockLds {
    double q[BI_CP][4], t[BI_CP][3], kn[BI_KN], seg[2 * BI_SEG_LDS];
    uint32_t plan[8];
};

// what every thread of the workgroup knows about its block after board_block_plan
struct BoardBlockPlan {
    int mode;                  // BI_NONE: no segment between the block's first and last time
    uint32_t g_blk, span_first, span_last;
    double seg_t0, seg_t1;     // staged: the segment's time range
    bool seg_lds;              // the segments' time ranges are in L.seg
    const double *qall, *tall;
};

// The block's plan, once per workgroup; every thread calls it (two barriers inside).  blk: the block's first record, count >= 1
// its events.  Wave 0 takes the block's first time, wave 1 its last: the first segment whose end is not below it, and the span
// of that time (clamped into the segment) there.
__device__ __forceinline__ BoardBlockPlan board_block_plan(const uint8_t *blk, uint32_t count, const BoardSpline &S, BoardBlockLds &L) {
    const int tid = threadIdx.x;
    BoardBlockPlan P;
    P.seg_lds = S.n_seg <= BI_SEG_LDS;
    if (P.seg_lds && (uint32_t) tid < 2 * S.n_seg) L.seg[tid] = S.seg_range[tid];
    if (tid < 128) {
        const int wv = tid >> 6;
        const double tq = bi_load_f64(blk + (size_t) (wv ? count - 1u : 0u) * 25);
        uint32_t g = bi_wave_count<false>(S.seg_range + 1, 2u, S.n_seg, tq);   // ends < tq
        bool any = g < S.n_seg;
        if (wv == 1 && (g == S.n_seg || tq < S.seg_range[2 * (size_t) g])) {     // the last time lies behind segment g - 1
            any = g > 0;
            g = g > 0 ? g - 1u : 0u;
        }
        uint32_t span = 3;
        if (any) {
            const double *kn = S.knots + S.knot_off[g];
            const uint32_t ncp = S.cp_off[g + 1] - S.cp_off[g];
            double tc = tq;
            tc = tc < kn[3] ? kn[3] : tc;
            tc = tc > kn[ncp] ? kn[ncp] : tc;
            span = 3u + bi_wave_count<true>(kn + 4, 1u, ncp - 4u, tc);           // the last span whose first knot is <= tc
        }
        if ((tid & 63) == 0) {
            L.plan[4 * wv] = any ? 1u : 0u;
            L.plan[4 * wv + 1] = g;
            L.plan[4 * wv + 2] = span;
        }
    }
    __syncthreads();
    P.mode = BI_GLOBAL;
    P.g_blk = L.plan[1];
    P.span_first = L.plan[2];
    P.span_last = L.plan[6];
    if (!L.plan[0] || !L.plan[4] || L.plan[1] > L.plan[5]) P.mode = BI_NONE;       // no segment between the block's first and last time
    else if (L.plan[1] == L.plan[5] && P.span_last >= P.span_first && P.span_last - P.span_first + 4u <= BI_CP) P.mode = BI_STAGED;
    P.qall = S.params + 9;
    P.tall = S.params + 9 + 4 * (size_t) S.n_cp_total;
    P.seg_t0 = 0.0;
    P.seg_t1 = 0.0;
    if (P.mode == BI_STAGED) {
        const uint32_t n_st = P.span_last - P.span_first + 4u, c0 = S.cp_off[P.g_blk] + P.span_first - 3u;
        const double *kn = S.knots + S.knot_off[P.g_blk] + (P.span_first - 3u);
        if ((uint32_t) tid < 4 * n_st) L.q[tid >> 2][tid & 3] = P.qall[4 * (size_t) c0 + tid];
        if ((uint32_t) tid < 3 * n_st) L.t[tid / 3][tid % 3] = P.tall[3 * (size_t) c0 + tid];
        if ((uint32_t) tid < n_st + 4u) L.kn[tid] = kn[tid];
        P.seg_t0 = S.seg_range[2 * (size_t) P.g_blk];
        P.seg_t1 = S.seg_range[2 * (size_t) P.g_blk + 1];
    }
    __syncthreads();
    return P;
}

// One event's pose inputs: the four basis values and the four control points of its span in the segment of its time (ranges
// inclusive, a shared time to the earlier segment, a NaN to none).  false: the time lies in no segment (b, q, t are not written).
// (No output for the segment's index: an out-parameter here cost the board image's kernels 6 - 22 VGPRs and one of them a wave
// per SIMD, although they never read it; bi_segment_of gives the same index where it is needed.)
__device__ __forceinline__ bool board_event_pose(const BoardBlockPlan &P, const BoardSpline &S, const BoardBlockLds &L, double et,
                                                 double b[4], double q[4][4], double t[4][3]) {
    bool in_time = false;
    if (P.mode == BI_STAGED) {
        in_time = et >= P.seg_t0 && et <= P.seg_t1;
        if (in_time) {
            uint32_t sp = P.span_first;
            while (sp < P.span_last && L.kn[sp + 1u - (P.span_first - 3u)] <= et) sp++;
            spline_basis(L.kn, sp - (P.span_first - 3u), et, b);
            const uint32_t j0 = sp - P.span_first;
            for (int j = 0; j < 4; j++) {
                for (int c = 0; c < 4; c++) q[j][c] = L.q[j0 + j][c];
                for (int c = 0; c < 3; c++) t[j][c] = L.t[j0 + j][c];
            }
        }
    } else if (P.mode == BI_GLOBAL) {
        const int g = bi_segment_of(et, P.seg_lds ? L.seg : S.seg_range, S.n_seg);
        in_time = g >= 0;
        if (in_time) {
            const double *kn = S.knots + S.knot_off[g];
            const uint32_t sp = spline_find_span(kn, S.cp_off[g + 1] - S.cp_off[g], et), c0 = S.cp_off[g] + sp - 3u;
            spline_basis(kn, sp, et, b);
            for (int j = 0; j < 4; j++) {
                for (int c = 0; c < 4; c++) q[j][c] = P.qall[4 * (size_t) (c0 + j) + c];
                for (int c = 0; c < 3; c++) t[j][c] = P.tall[3 * (size_t) (c0 + j) + c];
            }
        }
    }
    return in_time;
}

}  // namespace ecal
