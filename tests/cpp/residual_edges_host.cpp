// CPU harness (g++ -ffp-contract=off) of tests/test_residual_edges_host.py: evaluates the product's residual header
// (eventcalib_amd/csrc/spline_residual.hpp) and the oracle's dual-number functions (oracle/solver_oracle.cpp) on cases read
// from standard input and prints every value as a hexadecimal float, so that nothing is lost on the way to the high-precision
// comparison.  Test harness only: a stand-alone program, nothing is loaded into another process.
//
// input, per case (white space between the fields, doubles as C99 hexadecimal floats):
//   use_so3 fisheye | intr[9] | q[4][4] (xyzw) | t[4][3] | b[4] | obs[2] | lm[3] | radius
// output, per case: a line "P r J[0..32]" (the product) and a line "O r J[0..32]" (the oracle)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../eventcalib_amd/csrc/spline_residual.hpp"

extern "C" double oracle_residual_cam(const double *intr, const double *q4x4, const double *t4x3, const double *basis4,
                                      const double *obs2, const double *lm3, double radius, double *J37, double *J33, int fisheye);
extern "C" double oracle_residual_so3_cam(const double *intr, const double *q4x4, const double *t4x3, const double *basis4,
                                          const double *obs2, const double *lm3, double radius, double *J37, double *J33, int fisheye);

static bool read_double(double *out) {
    char tok[128];
    if (std::scanf("%127s", tok) != 1) return false;
    char *end = nullptr;
    *out = std::strtod(tok, &end);
    return end != tok && *end == 0;
}

static void print_row(const char *tag, double r, const double *J) {
    std::printf("%s %a", tag, r);
    for (int i = 0; i < 33; i++) std::printf(" %a", J[i]);
    std::printf("\n");
}

int main() {
    int n = 0;
    for (;;) {
        int so3 = 0, fisheye = 0;
        if (std::scanf("%d %d", &so3, &fisheye) != 2) break;
        double v[47];
        for (int i = 0; i < 47; i++)
            if (!read_double(&v[i])) {
                std::fprintf(stderr, "case %d: malformed input\n", n);
                return 1;
            }
        const double *intr = v, *qf = v + 9, *tf = v + 25, *b = v + 37, *obs = v + 41, *lm = v + 43;
        const double radius = v[46];
        double q[4][4], t[4][3];
        for (int j = 0; j < 4; j++) {
            for (int k = 0; k < 4; k++) q[j][k] = qf[4 * j + k];
            for (int k = 0; k < 3; k++) t[j][k] = tf[3 * j + k];
        }
        ecal::ResidualInput in;
        in.ifx = in.ify = 0.0;   // computed inside
        in.u = obs[0];
        in.v = obs[1];
        in.lmx = lm[0];
        in.lmy = lm[1];
        in.lmz = lm[2];
        in.radius = radius;
        for (int k = 0; k < 4; k++) in.b[k] = b[k];
        double J[33], Jo[33];
        double r;
        if (so3) r = fisheye ? ecal::spline_residual_so3<true>(in, intr, q, t, J) : ecal::spline_residual_so3<false>(in, intr, q, t, J);
        else r = fisheye ? ecal::spline_residual<true>(in, intr, q, t, J) : ecal::spline_residual<false>(in, intr, q, t, J);
        // the value-only call takes the same path up to the residual
        const double r0 = so3 ? (fisheye ? ecal::spline_residual_so3<true>(in, intr, q, t, nullptr) : ecal::spline_residual_so3<false>(in, intr, q, t, nullptr))
                              : (fisheye ? ecal::spline_residual<true>(in, intr, q, t, nullptr) : ecal::spline_residual<false>(in, intr, q, t, nullptr));
        if (std::memcmp(&r, &r0, sizeof r) != 0) {
            std::fprintf(stderr, "case %d: the residual differs with and without its row\n", n);
            return 2;
        }
        const double ro = (so3 ? oracle_residual_so3_cam : oracle_residual_cam)(intr, qf, tf, b, obs, lm, radius, nullptr, Jo, fisheye);
        print_row("P", r, J);
        print_row("O", ro, Jo);
        n++;
    }
    return n > 0 ? 0 : 3;
}
