// The sigma map of one pixel — one restatement of include/ecal_uncertainty.h, "sigma map", for the kernel (ecal_uncertainty.hip), the
// host entry point (ecal_uncertainty_map_host) and the CPU test (tests/test_uncertainty_map_host.py through that entry point).
//
// The ray of a pixel under the solver's inverse camera model, (X, Y) = (x, y) g(rho), its analytic Jacobian by the nine intrinsics
// and the propagation of a 9 x 9 covariance to the pixel: C = E cov E^T with E = diag(fx, fy) J, sigma_px = sqrt(lambda_max(C)).
// Every operation is one IEEE f64 operation rounded on its own and written in a fixed order: the translation units that include this
// header are built with -ffp-contract=off, so host and device agree bit for bit except through tan (FISHEYE).  Validity is
// ud_point's (undistort_point.hpp), asked of that function itself.
#pragma once
#include "undistort_point.hpp"

namespace ecal_uncertainty {

#define ECAL_UQ_HD ECAL_UD_HD

constexpr double UQ_SMALL_RHO_G = 1e-16;    // FISHEYE: g = P below (spline_residual.hpp, residual_ray)
constexpr double UQ_SMALL_RHO_DG = 1e-8;    // FISHEYE: g' = P' + P^3 / 3 below (residual_dc_dr2)

// J[18] = d (X, Y) / d (fx fy cx cy k1..k5), row-major 2 x 9; false: the pixel is invalid (J untouched)
ECAL_UQ_HD bool uq_ray_jacobian(int model, const double *intr, double u, double v, double *J) {
    ecal_undistort::Camera cam;
    cam.model = model;
    cam.reserved = 0;
    for (int i = 0; i < 9; i++) cam.intr[i] = intr[i];
    cam.out_k[0] = cam.out_k[1] = 1.0;
    cam.out_k[2] = cam.out_k[3] = 0.0;
    double X, Y;
    if (!ecal_undistort::ud_point(cam, u, v, &X, &Y)) return false;
    const double fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
    const double k1 = intr[4], k2 = intr[5], k3 = intr[6], k4 = intr[7], k5 = intr[8];
    const double x = (u - cx) / fx, y = (v - cy) / fy;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2, r10 = r8 * r2;
    const double P = ((((1.0 + k1 * r2) + k2 * r4) + k3 * r6) + k4 * r8) + k5 * r10;
    const double dP = (((k1 + (2.0 * k2) * r2) + (3.0 * k3) * r4) + (4.0 * k4) * r6) + (5.0 * k5) * r8;
    double g = P, dg = dP, sec2 = 1.0;
    if (model == ecal_undistort::UD_FISHEYE) {
        if (r2 > UQ_SMALL_RHO_G) {
            const double r = sqrt(r2), tn = tan(r * P);
            sec2 = 1.0 + tn * tn;
            g = tn / r;
        }
        if (r2 > UQ_SMALL_RHO_DG) dg = (sec2 * (0.5 * P + r2 * dP) - 0.5 * g) / r2;
        else dg = dP + ((P * P) * P) / 3.0;
    }
    // d (X, Y) / d (x, y)
    const double xy2 = (2.0 * (x * y)) * dg;
    const double Xx = g + (2.0 * (x * x)) * dg, Yy = g + (2.0 * (y * y)) * dg;
    // d x / d fx = -x / fx, d x / d cx = -1 / fx; y likewise
    const double xfx = -(x / fx), xcx = -(1.0 / fx), yfy = -(y / fy), ycy = -(1.0 / fy);
    J[0] = Xx * xfx;
    J[1] = xy2 * yfy;
    J[2] = Xx * xcx;
    J[3] = xy2 * ycy;
    J[9] = xy2 * xfx;
    J[10] = Yy * yfy;
    J[11] = xy2 * xcx;
    J[12] = Yy * ycy;
    const double pw[5] = {r2, r4, r6, r8, r10};
    for (int i = 0; i < 5; i++) {
        const double gk = sec2 * pw[i];     // d g / d k_i
        J[4 + i] = x * gk;
        J[13 + i] = y * gk;
    }
    return true;
}

// sqrt of the larger eigenvalue of C = E cov E^T, E = diag(fx, fy) J
ECAL_UQ_HD double uq_sigma_px(const double *intr, const double *J, const double *cov) {
    double E[18];
    for (int i = 0; i < 9; i++) {
        E[i] = intr[0] * J[i];
        E[9 + i] = intr[1] * J[9 + i];
    }
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = 0; i < 9; i++) {
        double s0 = 0.0, s1 = 0.0;     // (cov E0^T)[i], (cov E1^T)[i]
        for (int j = 0; j < 9; j++) {
            s0 = s0 + cov[9 * i + j] * E[j];
            s1 = s1 + cov[9 * i + j] * E[9 + j];
        }
        a = a + E[i] * s0;
        b = b + E[i] * s1;
        c = c + E[9 + i] * s1;
    }
    const double m = 0.5 * (a + c), h = 0.5 * (a - c);
    const double lam = m + sqrt(h * h + b * b);
    if (lam > 0.0) return sqrt(lam);
    return lam == lam ? 0.0 : lam;   // (a NaN covariance stays visible as NaN)
}

// one pixel of the map: *sigma = 0 and 1 is returned where the pixel is invalid
ECAL_UQ_HD uint8_t uq_pixel(int model, const double *intr, const double *cov, double u, double v, double *sigma, double *J_out) {
    double J[18];
    if (!uq_ray_jacobian(model, intr, u, v, J)) {
        *sigma = 0.0;
        if (J_out)
            for (int i = 0; i < 18; i++) J_out[i] = 0.0;
        return 1;
    }
    *sigma = uq_sigma_px(intr, J, cov);
    if (J_out)
        for (int i = 0; i < 18; i++) J_out[i] = J[i];
    return 0;
}

}  // namespace ecal_uncertainty
