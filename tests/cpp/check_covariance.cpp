// The covariance of the intrinsics from the banded-arrow system (eventcalib_amd/csrc/arrow_covariance.hpp) on the CPU, against a dense
// long double inverse.  tests/test_covariance_host.py builds this plainly and under AddressSanitizer + UndefinedBehaviorSanitizer
// (a stand-alone program with its own main: nothing is preloaded).
//
// The systems: H = J^T J of random rows with the solver's sparsity (a row touches the nine intrinsics and four consecutive control
// points), columns of very different magnitudes, packed into the accumulation layout the kernel writes (arrow_layout.hpp); n_cp = 4,
// 5, 9, 40.  What is compared, in the Jacobi-scaled system the factorisation runs in (Hs = D H D, D = diag(1 / (1 + sqrt(diag)))):
//   Sigma_ii and P = (H^-1)[intr, :]   |error| <= bar * max |Hs^-1|,   bar = 100 n eps kappa_2(Hs)
//   cov_robust                         |error| <= (2 bar + bar^2) G / (G - 1) sum_c B_c^2,   B_c = max |Hs^-1| * |D g_c|_1
// The first is the usual bound of an inverse through a Cholesky factor with a generous constant.  The second follows from it: s_c =
// P g_c carries an error of at most bar * B_c and is itself at most B_c, so s_c s_c^T carries at most (2 bar + bar^2) B_c^2.
// kappa_2 comes from power iterations on the dense Hs and on its dense inverse: they approach the extreme eigenvalues from inside,
// so the kappa used is never above the true one.
// Also: a control point without rows gives positive_definite = 0 and NaN; one cluster gives robust_valid = 0; n_res <= n_unknowns
// gives formal_valid = 0.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <random>
#include <thread>
#include <vector>
#include <sched.h>
#include <time.h>

#include "ecal.h"
#include "ecal_uncertainty.h"
#include "arrow_layout.hpp"
using namespace ecal;
namespace {
#include "arrow_host.hpp"
#include "arrow_covariance.hpp"

int fails = 0;
#define CHECK(cond, ...)                             \
    do {                                             \
        if (!(cond)) {                               \
            fails++;                                 \
            fprintf(stderr, "FAILED: " __VA_ARGS__); \
            fprintf(stderr, "\n");                   \
        }                                            \
    } while (0)

typedef long double ld;
constexpr double EPS = 2.220446049250313e-16;   // 2^-52

struct System {
    uint32_t n_cp = 0;
    size_t n = 0;                      // 6 n_cp + 9, control points first (ArrowSystem's order)
    std::vector<double> H;             // dense [n][n]
    std::vector<double> accum;         // the kernel's layout
    std::vector<ScoreChunk> chunks;
    std::vector<double> score;         // [chunks][33]
    uint64_t n_res = 0;
};

// score / Jacobian column -> index of the full tangent vector
size_t full_index(int col, uint32_t cp0, size_t nc) {
    if (col < 9) return nc + col;
    if (col < 21) return 6 * (size_t) (cp0 + (col - 9) / 3) + (col - 9) % 3;
    return 6 * (size_t) (cp0 + (col - 21) / 3) + 3 + (col - 21) % 3;
}

// spans: the first control point of every span that has rows; rows_per_span rows each, split into `pieces` chunks
System make_system(uint32_t n_cp, const std::vector<uint32_t> &spans, int rows_per_span, int pieces, uint32_t seed) {
    System S;
    S.n_cp = n_cp;
    const size_t nc = 6 * (size_t) n_cp;
    S.n = nc + 9;
    S.H.assign(S.n * S.n, 0.0);
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N(0.0, 1.0);
    // column magnitudes as in the solver: focal lengths ~1e-2 per unit, k5 ~1e2, rotations ~1e1, translations ~1e-1
    const double mag[33] = {1e-2, 1e-2, 3e-2, 3e-2, 1.0, 3.0, 10.0, 30.0, 100.0, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
                            0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1};
    double cost = 0.0;
    for (uint32_t cp0 : spans) {
        for (int p = 0; p < pieces; p++) {
            const int rows = rows_per_span / pieces + (p == 0 ? rows_per_span % pieces : 0);
            double sc[33] = {0};
            for (int r = 0; r < rows; r++) {
                double J[33];
                for (int i = 0; i < 33; i++) J[i] = mag[i] * N(rng);
                const double res = 0.05 * N(rng);
                cost += 0.5 * res * res;
                for (int i = 0; i < 33; i++) {
                    sc[i] += res * J[i];
                    for (int j = 0; j < 33; j++) S.H[full_index(i, cp0, nc) * S.n + full_index(j, cp0, nc)] += J[i] * J[j];
                }
            }
            S.chunks.push_back(ScoreChunk{cp0, (uint32_t) rows, 0u, cp0 + 3u});
            S.score.insert(S.score.end(), sc, sc + 33);
            S.n_res += (uint64_t) rows;
        }
    }
    // pack: [0] cost | [1..9] g_intr | [10..90] H_intr upper | per control point c: g_c[6] | H_c,intr[6][9] | H_c,c+d[4][6][6]
    S.accum.assign(ACC_HEAD + ACC_PER_CP * (size_t) n_cp, 0.0);
    S.accum[0] = cost;
    for (int i = 0; i < 9; i++)
        for (int j = i; j < 9; j++) S.accum[10 + 9 * i + j] = S.H[(nc + i) * S.n + nc + j];
    for (uint32_t c = 0; c < n_cp; c++) {
        double *b = &S.accum[ACC_HEAD + ACC_PER_CP * (size_t) c];
        for (int k = 0; k < 6; k++)
            for (int j = 0; j < 9; j++) b[6 + 9 * k + j] = S.H[(6 * (size_t) c + k) * S.n + nc + j];
        for (uint32_t d = 0; d < 4 && c + d < n_cp; d++)
            for (int ka = 0; ka < 6; ka++)
                for (int kb = 0; kb < 6; kb++) {
                    if (d == 0 && kb < ka) continue;
                    b[60 + 36 * d + 6 * ka + kb] = S.H[(6 * (size_t) c + ka) * S.n + 6 * (size_t) (c + d) + kb];
                }
    }
    return S;
}

// dense inverse of a symmetric positive definite matrix in long double (Cholesky); false: not positive definite
bool dense_inverse(const std::vector<double> &H, size_t n, std::vector<ld> &X) {
    std::vector<ld> C(n * n, 0.0L);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j <= i; j++) {
            ld v = H[i * n + j];
            for (size_t k = 0; k < j; k++) v -= C[i * n + k] * C[j * n + k];
            if (i == j) {
                if (!(v > 0.0L)) return false;
                C[i * n + i] = sqrtl(v);
            } else {
                C[i * n + j] = v / C[j * n + j];
            }
        }
    X.assign(n * n, 0.0L);
    std::vector<ld> x(n);
    for (size_t c = 0; c < n; c++) {
        for (size_t i = 0; i < n; i++) {
            ld v = i == c ? 1.0L : 0.0L;
            for (size_t k = 0; k < i; k++) v -= C[i * n + k] * x[k];
            x[i] = v / C[i * n + i];
        }
        for (size_t i = n; i-- > 0;) {
            ld v = x[i];
            for (size_t k = i + 1; k < n; k++) v -= C[k * n + i] * x[k];
            x[i] = v / C[i * n + i];
        }
        for (size_t i = 0; i < n; i++) X[i * n + c] = x[i];
    }
    return true;
}

// the largest eigenvalue of a symmetric positive definite matrix by power iteration (a Rayleigh quotient: never above the truth)
template <typename F>
double power_iteration(const F &at, size_t n) {
    std::vector<double> v(n), w(n);
    for (size_t i = 0; i < n; i++) v[i] = 1.0 + 0.37 * std::sin(1.0 + (double) i);
    double lam = 0.0;
    for (int it = 0; it < 400; it++) {
        double nv = 0.0, rq = 0.0;
        for (size_t i = 0; i < n; i++) {
            double s = 0.0;
            for (size_t j = 0; j < n; j++) s += at(i, j) * v[j];
            w[i] = s;
            rq += v[i] * s;
            nv += v[i] * v[i];
        }
        lam = rq / nv;
        double nw = 0.0;
        for (size_t i = 0; i < n; i++) nw += w[i] * w[i];
        nw = std::sqrt(nw);
        for (size_t i = 0; i < n; i++) v[i] = w[i] / nw;
    }
    return lam;
}

void check_system(const char *name, const System &S, uint32_t cluster_spans) {
    const size_t n = S.n, nc = n - 9;
    ecal_uncertainty_result out;
    arrow_uncertainty(S.accum.data(), S.n_cp, S.n_res, S.chunks.data(), S.score.data(), (uint32_t) S.chunks.size(), cluster_spans, &out);
    CHECK(out.positive_definite == 1, "%s: positive_definite", name);
    if (!out.positive_definite) return;
    // the library's own pieces again, for P
    ArrowSystem A;
    ArrowWorkspace ws;
    unpack(S.accum.data(), S.n_cp, A);
    IntrinsicsInverse R;
    CHECK(arrow_intrinsics_inverse(A, ws, R), "%s: arrow_intrinsics_inverse", name);
    std::vector<ld> X;
    CHECK(dense_inverse(S.H, n, X), "%s: the dense system is positive definite", name);
    const std::vector<double> &D = R.scale;
    for (size_t i = 0; i < n; i++) {
        const double h = S.H[i * n + i];
        CHECK(D[i] == 1.0 / (1.0 + std::sqrt(h)), "%s: scale[%zu]", name, i);
    }
    const double lmax = power_iteration([&](size_t i, size_t j) { return D[i] * S.H[i * n + j] * D[j]; }, n);
    const double imin = power_iteration([&](size_t i, size_t j) { return (double) (X[i * n + j] / ((ld) D[i] * D[j])); }, n);
    const double kappa = lmax * imin, bar = 100.0 * (double) n * EPS * kappa;
    ld M = 0.0L;   // max |Hs^-1|
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) M = std::max(M, fabsl(X[i * n + j] / ((ld) D[i] * D[j])));
    ld eS = 0.0L, eP = 0.0L;
    for (int i = 0; i < 9; i++) {
        for (int j = 0; j < 9; j++)
            eS = std::max(eS, fabsl((ld) R.Sii[9 * i + j] - X[(nc + i) * n + nc + j]) / ((ld) D[nc + i] * D[nc + j]));
        for (size_t k = 0; k < n; k++) eP = std::max(eP, fabsl((ld) R.P[(size_t) i * n + k] - X[(nc + i) * n + k]) / ((ld) D[nc + i] * D[k]));
    }
    // the robust covariance from the dense inverse
    std::vector<uint64_t> ids;
    for (const ScoreChunk &c : S.chunks) ids.push_back(((uint64_t) c.seg << 32) | ((c.span - 3) / cluster_spans));
    std::vector<uint64_t> uniq(ids);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const size_t G = uniq.size();
    std::vector<ld> cov(81, 0.0L);
    ld B2 = 0.0L;
    for (uint64_t id : uniq) {
        std::vector<ld> g(n, 0.0L);
        for (size_t c = 0; c < S.chunks.size(); c++)
            if (ids[c] == id)
                for (int i = 0; i < 33; i++) g[full_index(i, S.chunks[c].cp0, nc)] += S.score[33 * c + i];
        ld s[9], g1 = 0.0L;
        for (size_t k = 0; k < n; k++) g1 += fabsl(g[k] * D[k]);
        for (int i = 0; i < 9; i++) {
            s[i] = 0.0L;
            for (size_t k = 0; k < n; k++) s[i] += X[(nc + i) * n + k] * g[k];
        }
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) cov[9 * i + j] += s[i] * s[j];
        B2 += (M * g1) * (M * g1);
    }
    printf("%-28s n %3zu kappa %.3e bar %.3e | Sigma_ii %.3e  P %.3e (of max |Hs^-1|)", name, n, kappa, bar, (double) (eS / M), (double) (eP / M));
    CHECK(eS <= bar * M, "%s: Sigma_ii error %.3Le above %.3Le", name, eS, (ld) bar * M);
    CHECK(eP <= bar * M, "%s: P error %.3Le above %.3Le", name, eP, (ld) bar * M);
    CHECK(out.n_clusters == G, "%s: %u clusters, expected %zu", name, out.n_clusters, G);
    if (G >= 2) {
        const ld f = (ld) G / (ld) (G - 1);
        ld eC = 0.0L;
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) eC = std::max(eC, fabsl((ld) out.cov_robust[9 * i + j] - f * cov[9 * i + j]) / ((ld) D[nc + i] * D[nc + j]));
        const ld lim = (2.0L * bar + (ld) bar * bar) * f * B2;
        printf("  cov_robust %.3e of its bound", (double) (eC / lim));
        CHECK(out.robust_valid == 1, "%s: robust_valid", name);
        CHECK(eC <= lim, "%s: cov_robust error %.3Le above %.3Le", name, eC, lim);
        for (int i = 0; i < 9; i++) {
            CHECK(out.sigma_robust[i] == std::sqrt(out.cov_robust[10 * i]), "%s: sigma_robust[%d]", name, i);
            CHECK(out.inflation[i] == out.sigma_robust[i] / out.sigma[i], "%s: inflation[%d]", name, i);
        }
    } else {
        CHECK(out.robust_valid == 0, "%s: robust_valid with %zu clusters", name, G);
        for (int i = 0; i < 81; i++) CHECK(std::isnan(out.cov_robust[i]), "%s: cov_robust[%d] is not NaN", name, i);
        for (int i = 0; i < 9; i++) CHECK(std::isnan(out.sigma_robust[i]) && std::isnan(out.inflation[i]), "%s: sigma_robust / inflation [%d]", name, i);
    }
    printf("\n");
    // the formal covariance is s2 Sigma_ii, to the bit
    CHECK(out.formal_valid == 1 && out.n_unknowns == n && out.n_res == S.n_res && out.cost == S.accum[0], "%s: counts", name);
    CHECK(out.s2 == 2.0 * S.accum[0] / (double) (S.n_res - n), "%s: s2", name);
    for (int i = 0; i < 81; i++) CHECK(out.cov[i] == out.s2 * R.Sii[i], "%s: cov[%d]", name, i);
    for (int i = 0; i < 9; i++) {
        CHECK(out.sigma[i] == std::sqrt(out.cov[10 * i]) && out.sigma[i] > 0.0, "%s: sigma[%d]", name, i);
        CHECK(std::fabs(out.corr[10 * i] - 1.0) <= 4 * EPS, "%s: corr[%d][%d]", name, i, i);
        for (int j = 0; j < 9; j++) CHECK(out.corr[9 * i + j] == out.corr[9 * j + i] && std::fabs(out.corr[9 * i + j]) <= 1.0 + 4 * EPS, "%s: corr[%d][%d]", name, i, j);
    }
}

std::vector<uint32_t> all_spans(uint32_t n_cp) {
    std::vector<uint32_t> s;
    for (uint32_t c = 0; c + 4 <= n_cp; c++) s.push_back(c);
    return s;
}

}  // namespace

int main() {
    const uint32_t sizes[4] = {4, 5, 9, 40};
    for (int k = 0; k < 4; k++) {
        char name[64];
        const System S = make_system(sizes[k], all_spans(sizes[k]), 120, k == 2 ? 3 : 1, 1000u + sizes[k]);
        snprintf(name, sizeof name, "n_cp %u, cluster_spans 1", sizes[k]);
        check_system(name, S, 1);
        snprintf(name, sizeof name, "n_cp %u, cluster_spans 2", sizes[k]);
        check_system(name, S, 2);
        snprintf(name, sizeof name, "n_cp %u, one cluster", sizes[k]);
        check_system(name, S, 1000);   // G = 1: robust_valid = 0
    }
    {   // a control point whose rows are zero: spans at control points 0 and 5 of 9 leave control point 4 without a row
        const System S = make_system(9, {0u, 5u}, 120, 1, 77u);
        ecal_uncertainty_result out;
        arrow_uncertainty(S.accum.data(), S.n_cp, S.n_res, S.chunks.data(), S.score.data(), (uint32_t) S.chunks.size(), 1, &out);
        CHECK(out.positive_definite == 0 && out.formal_valid == 0 && out.robust_valid == 0, "empty control point: flags");
        CHECK(out.cost == S.accum[0] && out.n_res == S.n_res && out.n_unknowns == 63, "empty control point: counts");
        bool all_nan = std::isnan(out.s2);
        for (int i = 0; i < 81; i++) all_nan = all_nan && std::isnan(out.cov[i]) && std::isnan(out.corr[i]) && std::isnan(out.cov_robust[i]);
        for (int i = 0; i < 9; i++) all_nan = all_nan && std::isnan(out.sigma[i]) && std::isnan(out.sigma_robust[i]) && std::isnan(out.inflation[i]);
        CHECK(all_nan, "empty control point: NaN everywhere");
        printf("%-28s positive_definite 0, NaN everywhere\n", "empty control point");
    }
    {   // fewer residuals than unknowns cannot be positive definite from rows alone: a positive definite H with n_res <= n_unknowns
        System S = make_system(4, all_spans(4), 120, 1, 5u);
        S.n_res = S.n;
        ecal_uncertainty_result out;
        arrow_uncertainty(S.accum.data(), S.n_cp, S.n_res, S.chunks.data(), S.score.data(), (uint32_t) S.chunks.size(), 1, &out);
        CHECK(out.positive_definite == 1 && out.formal_valid == 0 && std::isnan(out.s2) && std::isnan(out.sigma[0]) && std::isnan(out.cov[0]),
              "n_res == n_unknowns: formal_valid");
        printf("%-28s formal_valid 0\n", "n_res == n_unknowns");
    }
    if (fails) {
        printf("check_covariance: %d FAILED\n", fails);
        return 1;
    }
    printf("check_covariance: ok\n");
    return 0;
}
