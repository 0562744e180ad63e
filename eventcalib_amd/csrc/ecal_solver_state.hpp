// The solver object and its device records, shared by the translation units that launch kernels over them: ecal_solver.hip
// (normal equations, Levenberg-Marquardt), ecal_report.hip (the calibration quality report) and ecal_board_image.hip.  Not part of the public ABI.
#pragma once
#include <memory>
#include <vector>
#include "ecal_ctx.hpp"
#include "arrow_layout.hpp"
#include "spline_residual.hpp"   // (a unit that contracts the residual to FMA by pragma includes it first, under its pragma)

namespace ecal {

struct ResRecord {  // 32 bytes per residual: the algorithmic traffic unit of SURVEY §8(d)
    double u, v, t;
    uint32_t lm, seg;
};
struct Chunk {
    uint32_t start, count, seg, span;
};

constexpr int NE_T = 256;   // threads per workgroup = rows per batch
constexpr uint32_t NE_CHUNK = 16384;  // residuals per workgroup (one span): few, long chunks keep the FP64 atomics rare

// A streamed evaluation (ecal_solver_solve, one rank, a long spline): the host factorises the interiors of its partition of the
// control points (arrow_host_parts.hpp) WHILE the kernel is still accumulating the later ones.  The chunks are ordered by knot
// span, i.e. by control point; group g = the chunks whose span's last control point lies in [cut[g], cut[g + 1]).  A chunk
// with last control point s adds to the records s - 3 .. s, so the records of interior g ([cut[g], cut[g + 1] - 3)) are touched
// by group g alone and the three records of the separator behind it by groups g and g + 1.  The workgroup that finishes a group
// (a counter per group) copies the interior's records into the host's pinned buffer and raises the group's flag there; the
// second of the two groups beside a separator to finish does the same for the separator's records.  The counters are restored
// by the workgroup that zeroes them: nothing to prepare per launch.
// (NE_MAX_GROUPS: arrow_layout.hpp)
struct NeProgress {
    uint32_t n_groups, n_cp;
    uint32_t cut[NE_MAX_GROUPS + 1];      // cut[n_groups] = n_cp
    uint32_t init[2 * NE_MAX_GROUPS];     // [g]: chunks of group g; [NE_MAX_GROUPS + b]: groups with chunks beside separator b
    uint32_t *left;                       // the running counters, same layout (device memory)
    double *host_acc;                     // the pinned accumulation buffer as the device sees it
    uint32_t *host_flag;                  // pinned; [g] / [NE_MAX_GROUPS + b] = number of the evaluation that delivered them
};

}  // namespace ecal

namespace ecal {
// the segments' time ranges from the solver's knots: [n_seg][2] = (knots_g[3], knots_g[n_cp_g])
inline std::vector<double> segment_time_ranges(const std::vector<double> &knots, const std::vector<uint32_t> &knot_off,
                                               const std::vector<uint32_t> &cp_off) {
    std::vector<double> r;
    for (size_t g = 0; g + 1 < cp_off.size(); g++) {
        r.push_back(knots[knot_off[g] + 3]);
        r.push_back(knots[knot_off[g] + (cp_off[g + 1] - cp_off[g])]);
    }
    return r;
}
}  // namespace ecal

struct ecal_solver {
    ecal_ctx *ctx = nullptr;
    uint64_t n_res = 0;
    uint32_t n_cp = 0, n_seg = 0, n_chunks = 0, n_lm = 0;
    double radius = 0, huber_a = 0;
    bool use_so3 = false;  // cumulative SO3 spline + LocalParameterizationSO3 instead of the quaternion spline
    bool fisheye = false;  // camera_model == ECAL_CAMERA_FISHEYE
    std::vector<uint32_t> cp_off, knot_off;
    std::vector<double> knots;
    std::vector<double> landmarks;   // host copy [n_lm][3] (ecal_board_image_default_options)
    ecal::ResRecord *d_rec = nullptr;
    ecal::Chunk *d_chunks = nullptr;
    double *d_knots = nullptr, *d_landmarks = nullptr, *d_params = nullptr, *d_accum = nullptr, *d_heads = nullptr;
    uint32_t *d_knot_off = nullptr, *d_cp_off = nullptr;
    double *d_seg_range = nullptr;   // [n_seg][2]: (knots_g[3], knots_g[n_cp_g]), the time range of every segment (ecal_board_image.hip)
    // ecal_solver_solve's pinned staging (kept: pinning 3 MB per solve costs more than an LM iteration) and the streamed
    // evaluation's progress block (NeProgress)
    double *h_acc = nullptr, *h_x = nullptr;
    uint32_t *h_flag = nullptr, *d_left = nullptr;
    ecal::NeProgress *d_prog = nullptr;
    ecal::NeProgress prog{};             // the host's copy (prog.n_groups = 0: not set up)
    std::shared_ptr<void> host_pool;   // ecal_solver_solve's worker threads (HostPool), parked between solves
    int host_pool_workers = -1;
    uint32_t stream_epoch = 0;
    uint32_t last_solve[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ecal_debug_solver_last_solve: how the last ecal_solver_solve ran
    size_t report_lds = 0;   // ecal_solver_report_dev: the dynamic LDS its kernel has been allowed so far
    size_t board_lds = 0;    // ecal_solver_board_image_dev: the same
    size_t report_px_lds = 0;   // ecal_solver_report_px_dev: the same
    size_t n_params() const { return 9 + 7 * (size_t) n_cp; }
    size_t n_accum() const { return ecal::ACC_HEAD + ecal::ACC_PER_CP * (size_t) n_cp; }
};

#if defined(__HIPCC__)
namespace ecal {
// One record into the residual's input: pixel, landmark, radius, 1 / fx, 1 / fy and the basis values at the record's time (kn, span,
// binv: the chunk's knots and span inverses).  The robust-loss fields stay with the caller.  Used by residual_rows_kernel,
// report_kernel and both kernels of ecal_report_px.hip; normal_eq_kernel writes these lines out, because six of its eight
// instantiations move with the call (design/08_solver.md, "One copy of the residual's pieces").
__device__ __forceinline__ void residual_input_fill(ResidualInput &in, const ResRecord &e, const double *landmarks, double radius,
                                                    double ifx, double ify, const double *kn, uint32_t span, const double binv[6]) {
    in.u = e.u;
    in.v = e.v;
    in.lmx = landmarks[3 * (size_t) e.lm];
    in.lmy = landmarks[3 * (size_t) e.lm + 1];
    in.lmz = landmarks[3 * (size_t) e.lm + 2];
    in.radius = radius;
    in.ifx = ifx;
    in.ify = ify;
    spline_basis_inv(kn, span, binv, e.t, in.b);
}

// the chunk's constants: intrinsics, span inverses, the four control points.  The kernels of ecal_report_px.hip and
// ecal_uncertainty.hip load them through this; the solver's own kernels write the same lines out (ecal_solver.hip says why).
struct ChunkPose {
    double q[4][4], t[4][3], pin[9], binv[6], ifx, ify;
    const double *kn;
    __device__ __forceinline__ void load(const Chunk &ch, const double *knots, const uint32_t *knot_off, const uint32_t *cp_off,
                                         const double *params, uint32_t n_cp_total) {
        kn = knots + knot_off[ch.seg];
        const uint32_t c0 = cp_off[ch.seg] + ch.span - 3;
        const double *qall = params + 9;
        const double *tall = params + 9 + 4 * (size_t) n_cp_total;
        for (int i = 0; i < 9; i++) pin[i] = params[i];
        spline_span_inverses(kn, ch.span, binv);
        ifx = 1.0 / pin[0];
        ify = 1.0 / pin[1];
        for (int j = 0; j < 4; j++) {
            for (int k = 0; k < 4; k++) q[j][k] = qall[4 * (size_t) (c0 + j) + k];
            for (int k = 0; k < 3; k++) t[j][k] = tall[3 * (size_t) (c0 + j) + k];
        }
    }
};
}  // namespace ecal
#endif
