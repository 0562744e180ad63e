// The deciding half of the board-frame passes (ecal_board_image.hip's ring profile, ecal_reassociate.hip's gate): the landmark
// nearest to a board point and the signed distance to its circle's rim.  Plain functions, usable from HIP kernels and host C++
// (tests/cpp/check_board_nearest.cpp).  They DECIDE, so they are compiled WITHOUT contraction to FMA: include this header
// where `fp contract(off)` is in force (the device translation units' default; -ffp-contract=off on the host).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef ECAL_HD
#if defined(__HIPCC__)
#define ECAL_HD __host__ __device__ __forceinline__
#else
#define ECAL_HD inline
#endif
#endif

namespace ecal {

constexpr uint32_t BOARD_NOT_KEPT = 0xFFu;   // the verdict byte of an event that is no residual; landmark indices stay below 128

ECAL_HD double board_sqrt_rn(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}

// the landmark (lm [n_lm][2], board units) with the smallest squared distance to (x, y) in the plane, ties to the lower index;
// *best = that squared distance (infinity, index 0, when there is no landmark or no distance compares below infinity: NaN)
ECAL_HD uint32_t board_nearest(const double *lm, uint32_t n_lm, double x, double y, double *best_out) {
    double best = (double) INFINITY;
    uint32_t bi = 0;
    for (uint32_t i = 0; i < n_lm; i++) {
        const double dx = x - lm[2 * i], dy = y - lm[2 * i + 1];
        const double d2 = dx * dx + dy * dy;
        if (d2 < best) {
            best = d2;
            bi = i;
        }
    }
    *best_out = best;
    return bi;
}

// the re-association's verdict on a board point: the nearest landmark's index when |d| < ring_tol with d = sqrt(best) - radius
// (*d_out), BOARD_NOT_KEPT otherwise (a NaN anywhere is not kept)
ECAL_HD uint32_t board_ring_gate(const double *lm, uint32_t n_lm, double x, double y, double radius, double ring_tol, double *d_out) {
    double best;
    const uint32_t bi = board_nearest(lm, n_lm, x, y, &best);
    const double d = board_sqrt_rn(best) - radius;
    *d_out = d;
    return fabs(d) < ring_tol ? bi : BOARD_NOT_KEPT;
}

}  // namespace ecal
