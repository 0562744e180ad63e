// CPU check (g++): spline_residual_px / spline_residual_px_so3 / residual_px_distance (eventcalib_amd/csrc/spline_residual.hpp) —
// the residual with its gradient by the event's own pixel, the lean pair behind the report in pixels — against the residual
// functions themselves.  Both are built on the same helpers of one header (residual_ray, residual_distance, residual_ray_back,
// residual_dc_dr2, the pose functions) with one set of flags (-ffp-contract=off); what each adds — the robust loss and the row in
// residual_core, the two lines that form gx, gy in both — must leave r equal to spline_residual*'s value and (gu, gv) to the
// negated columns 2 and 3 of the same call's Jacobian row BIT FOR BIT, and the degenerate verdict must be "r or g2 is not finite,
// or g2 > 0 is false" exactly.  That the shared arithmetic is what it was: residual_frozen.cpp.  Test harness only; stand-alone
// (its own main), so it can also be built with -fsanitize=address,undefined and run as it is.
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

// the verdict and the distance by the stated rule, with <cmath>'s classification instead of the header's comparisons
static bool rule(double r, double gu, double gv, double *r_px, double *ppu) {
    const double a = gu * gu, b = gv * gv;
    const double g2 = a + b;
    *r_px = 0.0;
    *ppu = 0.0;
    if (!std::isfinite(r) || !std::isfinite(g2) || !(g2 > 0.0)) return true;
    const double n = std::sqrt(g2);
    *r_px = r / n;
    *ppu = 1.0 / n;
    return false;
}

static int check_distance(const char *what, double r, double gu, double gv, int want_degenerate /* -1: whatever the rule says */) {
    const double g[2] = {gu, gv};
    double mine, mine_ppu, ref, ref_ppu;
    const bool deg = ecal::residual_px_distance(r, g, &mine, &mine_ppu);
    const bool ref_deg = rule(r, gu, gv, &ref, &ref_ppu);
    if (deg != ref_deg || (want_degenerate >= 0 && deg != (want_degenerate != 0))) {
        std::printf("%s: r %.17g g (%.17g, %.17g): verdict %d, the rule says %d\n", what, r, gu, gv, (int) deg, (int) ref_deg);
        return 1;
    }
    if (bits(mine) != bits(ref) || bits(mine_ppu) != bits(ref_ppu)) {
        std::printf("%s: r_px %.17g (rule %.17g), px_per_unit %.17g (rule %.17g)\n", what, mine, ref, mine_ppu, ref_ppu);
        return 1;
    }
    if (deg && (mine != 0.0 || mine_ppu != 0.0)) {
        std::printf("%s: a degenerate record must come out as zeros\n", what);
        return 1;
    }
    return 0;
}

template <bool SO3, bool FISHEYE>
static int one_case(std::mt19937_64 &rng, int trial, int *n_ok, int *n_deg) {
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
    double base[4] = {0.05 * U(rng), 0.05 * U(rng), 0.7 + 0.05 * U(rng), 0.7 + 0.05 * U(rng)};
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
    ecal::ResidualInput in;
    // 1 / fx, 1 / fy handed in (as the kernels do) on some trials, computed inside on the others
    in.ifx = trial & 4 ? 0.0 : 1.0 / intr[0];
    in.ify = trial & 4 ? 0.0 : 1.0 / intr[1];
    in.u = 173 + 150 * U(rng);
    in.v = 130 + 110 * U(rng);
    in.lmx = 19 + 18 * U(rng);
    in.lmy = 22 + 20 * U(rng);
    in.lmz = 0;
    in.radius = 1.75;
    // every 16th case a pixel that is not a number: r and the gradient come out NaN in both functions
    if (trial % 16 == 9) in.u = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 4; k++) in.b[k] = b[k];

    double J[ecal::RES_NJ], g[2];
    const double r_plain = SO3 ? ecal::spline_residual_so3<FISHEYE>(in, intr, q, t, nullptr) : ecal::spline_residual<FISHEYE>(in, intr, q, t, nullptr);
    const double r_row = SO3 ? ecal::spline_residual_so3<FISHEYE>(in, intr, q, t, J) : ecal::spline_residual<FISHEYE>(in, intr, q, t, J);
    const double r = SO3 ? ecal::spline_residual_px_so3<FISHEYE>(in, intr, q, t, g) : ecal::spline_residual_px<FISHEYE>(in, intr, q, t, g);
    if (bits(r) != bits(r_plain) || bits(r) != bits(r_row)) {
        std::printf("trial %d (so3 %d fisheye %d): r %.17g, the residual %.17g / %.17g\n", trial, (int) SO3, (int) FISHEYE, r, r_plain, r_row);
        return 1;
    }
    if (bits(g[0]) != bits(-J[2]) || bits(g[1]) != bits(-J[3])) {
        std::printf("trial %d (so3 %d fisheye %d): g (%.17g, %.17g), -J[2], -J[3] (%.17g, %.17g)\n", trial, (int) SO3, (int) FISHEYE, g[0], g[1],
                    -J[2], -J[3]);
        return 1;
    }
    if (check_distance("random case", r, g[0], g[1], trial % 16 == 9 ? 1 : 0)) return 1;
    (trial % 16 == 9 ? *n_deg : *n_ok)++;
    return 0;
}

// a board point EXACTLY on its landmark: the identity rotation, the pixel at the principal point, dyadic numbers throughout —
// Xw = (16, 24, 0) = the landmark, dd = 0, 1 / sqrt(0) = inf, r = 0 * inf - radius = NaN: degenerate
template <bool SO3, bool FISHEYE>
static int on_the_landmark() {
    const double intr[9] = {256.0, 256.0, 172.5, 129.5, FISHEYE ? -0.05 : 0.35, 0.02, -0.01, 0.0, 0.0};
    double q[4][4], t[4][3];
    for (int j = 0; j < 4; j++) {
        q[j][0] = q[j][1] = q[j][2] = 0.0;
        q[j][3] = 1.0;
        t[j][0] = 16.0;
        t[j][1] = 24.0;
        t[j][2] = -64.0;
    }
    ecal::ResidualInput in;
    in.ifx = in.ify = 0.0;
    in.u = 172.5;
    in.v = 129.5;
    in.lmx = 16.0;
    in.lmy = 24.0;
    in.lmz = 0.0;
    in.radius = 1.75;
    for (int k = 0; k < 4; k++) in.b[k] = 0.25;
    double J[ecal::RES_NJ], g[2];
    const double r_row = SO3 ? ecal::spline_residual_so3<FISHEYE>(in, intr, q, t, J) : ecal::spline_residual<FISHEYE>(in, intr, q, t, J);
    const double r = SO3 ? ecal::spline_residual_px_so3<FISHEYE>(in, intr, q, t, g) : ecal::spline_residual_px<FISHEYE>(in, intr, q, t, g);
    if (!std::isnan(r) || bits(r) != bits(r_row) || bits(g[0]) != bits(-J[2]) || bits(g[1]) != bits(-J[3])) {
        std::printf("on the landmark (so3 %d fisheye %d): r %.17g (row %.17g), g (%.17g, %.17g)\n", (int) SO3, (int) FISHEYE, r, r_row, g[0], g[1]);
        return 1;
    }
    return check_distance("on the landmark", r, g[0], g[1], 1);
}

static int verdict_edges() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double den = std::numeric_limits<double>::denorm_min();
    struct {
        double r, gu, gv;
        int want;
        const char *what;
    } cases[] = {
        {0.25, 0.03, -0.04, 0, "a plain record"},
        {-0.25, 0.0, 0.04, 0, "one component zero"},
        {0.0, 0.03, 0.04, 0, "a residual of zero"},
        {0.25, 0.0, 0.0, 1, "a gradient of zero: g2 > 0 is false"},
        {0.25, -0.0, 0.0, 1, "a gradient of minus zero"},
        {0.25, 1e-200, 1e-200, 1, "a gradient whose square underflows to zero"},
        {0.25, 1e-160, 0.0, 0, "a gradient whose square is a denormal: positive, so not degenerate"},
        {0.25, den, 0.0, 1, "the smallest denormal: its square is zero"},
        {0.25, 1e200, 0.0, 1, "a gradient whose square overflows"},
        {0.25, inf, 0.0, 1, "an infinite gradient"},
        {0.25, nan, 0.04, 1, "a NaN gradient"},
        {0.25, 0.03, nan, 1, "a NaN gradient (v)"},
        {nan, 0.03, 0.04, 1, "a NaN residual"},
        {inf, 0.03, 0.04, 1, "an infinite residual"},
        {-inf, 0.03, 0.04, 1, "a negative infinite residual"},
        {1e308, 0.03, 0.04, 0, "a huge finite residual"},
    };
    for (const auto &c : cases)
        if (check_distance(c.what, c.r, c.gu, c.gv, c.want)) return 1;
    // 3-4-5: r_px = 0.25 / 0.05 up to the rounding of the squares
    double r_px, ppu;
    const double g[2] = {0.03, -0.04};
    if (ecal::residual_px_distance(0.25, g, &r_px, &ppu) || std::fabs(r_px - 5.0) > 1e-14 || std::fabs(ppu - 20.0) > 1e-13) {
        std::printf("3-4-5: r_px %.17g px_per_unit %.17g\n", r_px, ppu);
        return 1;
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20261);
    int n_ok = 0, n_deg = 0;
    for (int trial = 0; trial < 10000; trial++) {
        int rc;
        switch (trial & 3) {
        case 0: rc = one_case<false, false>(rng, trial, &n_ok, &n_deg); break;
        case 1: rc = one_case<false, true>(rng, trial, &n_ok, &n_deg); break;
        case 2: rc = one_case<true, false>(rng, trial, &n_ok, &n_deg); break;
        default: rc = one_case<true, true>(rng, trial, &n_ok, &n_deg); break;
        }
        if (rc) return rc;
    }
    if (on_the_landmark<false, false>() || on_the_landmark<false, true>() || on_the_landmark<true, false>() || on_the_landmark<true, true>()) return 2;
    if (verdict_edges()) return 3;
    std::printf("residual px: 10000 cases bit-equal to the residual and its Jacobian row, %d with a distance, %d degenerate\n", n_ok, n_deg);
    return n_ok > 9000 && n_deg > 500 ? 0 : 4;
}
