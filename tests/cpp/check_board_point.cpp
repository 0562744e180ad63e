// CPU check (g++): spline_board_point / spline_pose_quat / spline_pose_so3 (eventcalib_amd/csrc/spline_residual.hpp) — the
// first half of the residual, which the board-frame event image uses on its own — against the residual functions.  They share
// residual_ray and the pose functions, so this is no longer a copy held to its original: what is checked is that the tail of
// the residual, reconstructed HERE from the board point (|Xw - lm| - radius on two coordinates), equals spline_residual*'s value
// BIT FOR BIT (one header, one set of flags), and that the verdict is "the depth is finite and positive" exactly, against a
// depth computed by another route in long double.  That the shared arithmetic is what it was: residual_frozen.cpp.  Test harness
// only; stand-alone (its own main), so it can also be built with -fsanitize=address,undefined and run as it is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include "../../eventcalib_amd/csrc/spline_residual.hpp"

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

// the depth by another route: third row of the rotation MATRIX of the normalised quaternion times the ray, in long double
template <bool FISHEYE>
static long double depth_ref(double u, double v, const double *intr, const double Q[4], const double T[3]) {
    const long double x = ((long double) u - intr[2]) / intr[0], y = ((long double) v - intr[3]) / intr[1];
    const long double r2 = x * x + y * y;
    long double poly = 1.0L, p = r2;
    for (int i = 4; i < 9; i++) {
        poly += intr[i] * p;
        p *= r2;
    }
    long double c = poly;
    if (FISHEYE && r2 > 1e-16L) {
        const long double r = std::sqrt(r2);
        c = std::tan(r * poly) / r;
    }
    const long double n = std::sqrt((long double) Q[0] * Q[0] + (long double) Q[1] * Q[1] + (long double) Q[2] * Q[2] + (long double) Q[3] * Q[3]);
    const long double qx = Q[0] / n, qy = Q[1] / n, qz = Q[2] / n, qw = Q[3] / n;
    const long double Y2 = 2 * (qx * qz - qw * qy) * (x * c) + 2 * (qy * qz + qw * qx) * (y * c) + (1 - 2 * (qx * qx + qy * qy));
    return -(long double) T[2] / Y2;
}

template <bool SO3, bool FISHEYE>
static int one_case(std::mt19937_64 &rng, int trial, int *n_false, int *n_true) {
    std::uniform_real_distribution<double> U(-1, 1);
    double intr[9] = {359.67525 + 20 * U(rng), 359.67525 + 20 * U(rng), 172.5 + 5 * U(rng), 129.5 + 5 * U(rng), 0, 0, 0, 0, 0};
    if (FISHEYE) {
        const double k[5] = {-0.05 + 0.02 * U(rng), 0.0175 + 0.01 * U(rng), -0.0075 + 0.005 * U(rng), 0.003 + 0.003 * U(rng), -0.001 + 0.002 * U(rng)};
        for (int i = 0; i < 5; i++) intr[4 + i] = k[i];
    } else {
        const double k[5] = {0.35 + 0.05 * U(rng), 0.38 + 0.05 * U(rng), -0.04 + 0.02 * U(rng), -1.16 + 0.1 * U(rng), -4.1 + 0.3 * U(rng)};
        for (int i = 0; i < 5; i++) intr[4 + i] = k[i];
    }
    double q[4][4], t[4][3], b[4];
    // every third case the camera looks AWAY from the board (half a turn about x on top of the usual attitude): negative depth
    const bool away = trial % 3 == 1;
    double base[4] = {0.05 * U(rng), 0.05 * U(rng), 0.7 + 0.05 * U(rng), 0.7 + 0.05 * U(rng)};
    if (away) {
        const double half_turn_x[4] = {1, 0, 0, 0}, in[4] = {base[0], base[1], base[2], base[3]};
        ecal::quat_mul(in, half_turn_x, base);
    }
    double nb = std::sqrt(base[0] * base[0] + base[1] * base[1] + base[2] * base[2] + base[3] * base[3]);
    for (int k = 0; k < 4; k++) base[k] /= nb;
    for (int j = 0; j < 4; j++) {
        if (SO3) {
            const double w[3] = {0.05 * U(rng), 0.05 * U(rng), 0.05 * U(rng)};
            ecal::so3_plus(j ? q[j - 1] : base, w, q[j]);
        } else {
            double n = 0;
            for (int k = 0; k < 4; k++) {
                q[j][k] = base[k] + 0.02 * U(rng);
                n += q[j][k] * q[j][k];
            }
            n = std::sqrt(n) * (1.0 + 0.01 * U(rng));   // control points are only approximately unit
            for (int k = 0; k < 4; k++) q[j][k] /= n;
        }
        t[j][0] = 19 + 3 * U(rng);
        t[j][1] = 22 + 3 * U(rng);
        t[j][2] = -66 + 5 * U(rng);
    }
    const double knots[11] = {0, 0, 0, 0, 0.21, 0.48, 0.77, 1, 1, 1, 1};
    const double u = 0.5 * (U(rng) + 1.0);
    ecal::spline_basis(knots, ecal::spline_find_span(knots, 7, u), u, b);
    const double obs[2] = {173 + 150 * U(rng), 130 + 110 * U(rng)};
    const double lm[3] = {19 + 18 * U(rng), 22 + 20 * U(rng), 0};
    const double radius = 1.75;
    // 1 / fx, 1 / fy handed in (as the kernels do) on even trials, computed inside on odd ones
    const double ifx = trial & 4 ? 0.0 : 1.0 / intr[0], ify = trial & 4 ? 0.0 : 1.0 / intr[1];

    ecal::ResidualInput in;
    in.ifx = ifx;
    in.ify = ify;
    in.u = obs[0];
    in.v = obs[1];
    in.lmx = lm[0];
    in.lmy = lm[1];
    in.lmz = lm[2];
    in.radius = radius;
    for (int k = 0; k < 4; k++) in.b[k] = b[k];
    const double res = SO3 ? ecal::spline_residual_so3<FISHEYE>(in, intr, q, t, nullptr) : ecal::spline_residual<FISHEYE>(in, intr, q, t, nullptr);

    double Q[4], T[3], Xw[2];
    if (SO3) ecal::spline_pose_so3(b, q, t, Q, T); else ecal::spline_pose_quat(b, q, t, Q, T);
    const bool ok = ecal::spline_board_point<FISHEYE>(obs[0], obs[1], intr, ifx, ify, Q[0], Q[1], Q[2], Q[3], T, Xw);
    // residual_core's tail on the two coordinates (its third difference, Xw_z - 0, is rounding noise of ~1e-14 whose square
    // cannot reach the last bit of the sum)
    const double d0 = Xw[0] - lm[0], d1 = Xw[1] - lm[1];
    const double dd = d0 * d0 + d1 * d1;
    const double mine = dd * ecal::res_rsqrt(dd) - radius;
    if (bits(mine) != bits(res)) {
        std::printf("trial %d (so3 %d fisheye %d): board point gives %.17g, the residual %.17g\n", trial, (int) SO3, (int) FISHEYE, mine, res);
        return 1;
    }
    const long double s = depth_ref<FISHEYE>(obs[0], obs[1], intr, Q, T);
    if (!(std::fabs(s) > 1e-6L)) {
        std::printf("trial %d: the generator made a depth of %Lg: the sign check needs a clear one\n", trial, s);
        return 1;
    }
    const bool want = std::isfinite((double) s) && s > 0;
    if (ok != want) {
        std::printf("trial %d (so3 %d fisheye %d): verdict %d at depth %Lg\n", trial, (int) SO3, (int) FISHEYE, (int) ok, s);
        return 1;
    }
    if (away != !ok) {
        std::printf("trial %d: a camera looking %s the board, verdict %d\n", trial, away ? "away from" : "at", (int) ok);
        return 1;
    }
    (ok ? *n_true : *n_false)++;
    return 0;
}

template <bool FISHEYE>
static int edge_cases() {
    const double intr[9] = {359.67525, 359.67525, 172.5, 129.5, FISHEYE ? -0.05 : 0.35, 0.02, -0.01, 0.0, 0.0};
    const double Q[4] = {0, 0, std::sqrt(0.5), std::sqrt(0.5)};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double Xw[2];
    struct {
        double u, v, T[3];
        bool want;
        const char *what;
    } cases[] = {
        {170.0, 130.0, {19, 22, -66}, true, "a plain view"},
        {170.0, 130.0, {19, 22, 0.0}, false, "the camera in the board plane: depth 0"},
        {170.0, 130.0, {19, 22, 66}, false, "the camera behind the board: negative depth"},
        {nan, 130.0, {19, 22, -66}, false, "a NaN pixel"},
        {170.0, 130.0, {19, 22, -inf}, false, "an infinite depth"},
        {170.0, 130.0, {19, 22, nan}, false, "a NaN translation"},
    };
    for (const auto &c : cases) {
        const bool ok = ecal::spline_board_point<FISHEYE>(c.u, c.v, intr, 0.0, 0.0, Q[0], Q[1], Q[2], Q[3], c.T, Xw);
        if (ok != c.want) {
            std::printf("edge case (fisheye %d) %s: verdict %d\n", (int) FISHEYE, c.what, (int) ok);
            return 1;
        }
    }
    // Y_z == 0 exactly: a quarter turn about x maps the optical axis into the plane; the pixel at the principal point
    const double Qx[4] = {std::sqrt(0.5), 0, 0, std::sqrt(0.5)}, T[3] = {19, 22, -66};
    const bool ok = ecal::spline_board_point<FISHEYE>(intr[2], intr[3], intr, 0.0, 0.0, Qx[0], Qx[1], Qx[2], Qx[3], T, Xw);
    const double Y2 = 1.0 - 2.0 * (Qx[0] * Qx[0]);   // what the function computes for p = (0, 0, 1)
    if (ok != (std::isfinite(66.0 / Y2) && 66.0 / Y2 > 0)) {
        std::printf("edge case (fisheye %d) ray along the plane: verdict %d with Y_z %g\n", (int) FISHEYE, (int) ok, Y2);
        return 1;
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20260);
    int n_false = 0, n_true = 0;
    for (int trial = 0; trial < 10000; trial++) {
        int rc;
        switch (trial & 3) {
        case 0: rc = one_case<false, false>(rng, trial, &n_false, &n_true); break;
        case 1: rc = one_case<false, true>(rng, trial, &n_false, &n_true); break;
        case 2: rc = one_case<true, false>(rng, trial, &n_false, &n_true); break;
        default: rc = one_case<true, true>(rng, trial, &n_false, &n_true); break;
        }
        if (rc) return rc;
    }
    if (edge_cases<false>() || edge_cases<true>()) return 2;
    std::printf("board point: 10000 cases bit-equal to the residual, %d in front, %d behind\n", n_true, n_false);
    return n_true > 3000 && n_false > 3000 ? 0 : 3;
}
