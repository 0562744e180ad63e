// CPU check (g++): board_nearest / board_ring_gate (eventcalib_amd/csrc/board_nearest.hpp) — the deciding half of the board-frame
// passes — against a straightforward loop: 10 000 random cases, a third of them on a lattice where EXACT ties are the rule (a point half way between
// lattice sites, repeated landmarks), some with no landmark, a
// NaN point or a point exactly on the gate.  Test harness only; stand-alone (its own main), so it can also be built with
// -fsanitize=address,undefined and run as it is.  Build with -ffp-contract=off, as the header asks.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "../../eventcalib_amd/csrc/board_nearest.hpp"

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

int main() {
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> coord(-10.0, 60.0), unit(0.0, 1.0);
    int ties = 0, kept = 0, empty = 0, nans = 0, on_gate = 0;
    for (int it = 0; it < 10000; it++) {
        const uint32_t n_lm = it % 50 == 0 ? 0u : 1u + (uint32_t) (rng() % 128);
        std::vector<double> lm(2 * (size_t) n_lm + 2);   // (+2: never an empty allocation; the function must not read them)
        for (uint32_t i = 0; i < n_lm; i++) {
            // an 8 x 8 lattice: differences and their squares are exact, so equal distances are exact ties
            lm[2 * i] = it % 3 == 0 ? (double) (int) (rng() % 8) : coord(rng);
            lm[2 * i + 1] = it % 3 == 0 ? (double) (int) (rng() % 8) : coord(rng);
        }
        if (n_lm > 3 && it % 6 == 0) {   // a repeated landmark
            lm[2 * (n_lm - 1)] = lm[0];
            lm[2 * (n_lm - 1) + 1] = lm[1];
        }
        double x = coord(rng), y = coord(rng);
        if (it % 3 == 0 && n_lm >= 2) {   // on the half lattice: two or four sites at exactly the same distance
            x = 0.5 * (double) (int) (rng() % 16);
            y = 0.5 * (double) (int) (rng() % 16);
        }
        if (it % 97 == 0) x = std::numeric_limits<double>::quiet_NaN();
        const double radius = 1.75;
        double tol = 0.05 + unit(rng);
        // the straightforward loop
        double best = std::numeric_limits<double>::infinity();
        uint32_t bi = 0;
        int n_best = 0;
        for (uint32_t i = 0; i < n_lm; i++) {
            const double dx = x - lm[2 * i], dy = y - lm[2 * i + 1], d2 = dx * dx + dy * dy;
            if (d2 < best) {
                best = d2;
                bi = i;
                n_best = 1;
            } else if (d2 == best) {
                n_best++;
            }
        }
        const double d = std::sqrt(best) - radius;
        if (it % 11 == 0 && std::isfinite(d)) tol = std::fabs(d);   // exactly on the gate: |d| < tol is false
        const uint32_t verdict = std::fabs(d) < tol ? bi : ecal::BOARD_NOT_KEPT;

        double got_best = -1.0, got_d = -1.0;
        const uint32_t got_bi = ecal::board_nearest(lm.data(), n_lm, x, y, &got_best);
        const uint32_t got_verdict = ecal::board_ring_gate(lm.data(), n_lm, x, y, radius, tol, &got_d);
        if (got_bi != bi || bits(got_best) != bits(best) || got_verdict != verdict || bits(got_d) != bits(d)) {
            std::printf("case %d: landmark %u / %u, best %.17g / %.17g, verdict %u / %u, d %.17g / %.17g\n", it, got_bi, bi, got_best, best,
                        got_verdict, verdict, got_d, d);
            return 1;
        }
        if (verdict != ecal::BOARD_NOT_KEPT && !(std::fabs(d) < tol && verdict < n_lm)) return 2;
        ties += n_best > 1;
        kept += verdict != ecal::BOARD_NOT_KEPT;
        empty += n_lm == 0;
        nans += x != x;
        on_gate += it % 11 == 0 && std::isfinite(d);
        if ((n_lm == 0 || x != x) && verdict != ecal::BOARD_NOT_KEPT) return 3;
        if (it % 11 == 0 && std::isfinite(d) && verdict != ecal::BOARD_NOT_KEPT) return 4;
    }
    std::printf("10000 cases equal: %d with exact ties, %d kept, %d without landmarks, %d NaN points, %d exactly on the gate\n", ties, kept,
                empty, nans, on_gate);
    return ties >= 1000 && kept >= 500 && empty > 0 && nans > 0 && on_gate > 0 ? 0 : 5;
}
