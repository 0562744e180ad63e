// Covariance of the intrinsics from the banded-arrow system (include/ecal_uncertainty.h, ecal_solver_uncertainty; the estimators:
// design/24_uncertainty.md).  Plain C++ — no HIP in here.  Included where arrow_host.hpp is, after it, inside the same namespace: it
// reuses ArrowSystem, unpack and solve_arrow's banded Cholesky (its factor L and Z = L^-1 [border | rhs] stay in the workspace).
// File-scope includes beside arrow_host.hpp's: <limits> "ecal_uncertainty.h".  tests/cpp/check_covariance.cpp compiles it with g++
// against a dense long double inverse, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#pragma once

// the rows of H^-1 that belong to the intrinsics, H the unpacked system with NO LM diagonal
struct IntrinsicsInverse {
    bool positive_definite = false;
    double Sii[81];           // (H^-1)[intr, intr] = the inverse of the 9 x 9 Schur complement
    std::vector<double> P;    // [9][nc + 9] = (H^-1)[intr, :] = [ -Sii W^T | Sii ], W = L^-T Z_b; columns in ArrowSystem's order:
                              // control point c at 6 c (rotation 3, translation 3), the intrinsics at nc
    std::vector<double> scale;   // the Jacobi scaling the factorisation ran in: 1 / (1 + sqrt(diag)), [nc + 9]
};

// false (and positive_definite = 0, nothing else to be used): a pivot of the banded part or of the Schur complement is not positive
inline bool arrow_intrinsics_inverse(const ArrowSystem &A, ArrowWorkspace &ws, IntrinsicsInverse &R) {
    const size_t nc = A.nc, nt = nc + 9;
    R.positive_definite = false;
    R.scale.resize(nt);
    for (size_t i = 0; i < nc; i++) R.scale[i] = 1.0 / (1.0 + std::sqrt(std::max(A.band[i * BW], 0.0)));
    for (int j = 0; j < 9; j++) R.scale[nc + j] = 1.0 / (1.0 + std::sqrt(std::max(A.corner[10 * j], 0.0)));
    const std::vector<double> dd(nt, 0.0);
    std::vector<double> y;
    ws.reduce_G = nullptr;
    if (!solve_arrow(A, R.scale, dd, y, ws)) return false;
    const double *sc = R.scale.data();
    const double *L = ws.L.data(), *Z = ws.Z.data(), *G = ws.G;
    // the scaled Schur complement (as solve_arrow forms it), its Cholesky factor and its inverse.  solve_arrow has formed and factorised
    // the same 9 x 9 matrix and solved for a step that is not wanted here: the duplication is deliberate, so that solve_arrow, the LM
    // loop's routine, stays as it is (the cost is nothing beside the banded factorisation)
    double S[81], Si[81];
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) S[9 * i + j] = A.corner[9 * i + j] * sc[nc + i] * sc[nc + j] - (i <= j ? G[10 * i + j] : G[10 * j + i]);
    for (int i = 0; i < 9; i++)
        for (int j = 0; j <= i; j++) {
            double v = S[9 * i + j];
            for (int k = 0; k < j; k++) v -= S[9 * i + k] * S[9 * j + k];
            if (i == j) {
                if (!(v > 0.0)) return false;
                S[9 * i + i] = std::sqrt(v);
            } else {
                S[9 * i + j] = v / S[9 * j + j];
            }
        }
    for (int c = 0; c < 9; c++) {   // column c of the inverse: C C^T x = e_c
        double x[9];
        for (int i = 0; i < 9; i++) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) v -= S[9 * i + k] * x[k];
            x[i] = v / S[9 * i + i];
        }
        for (int i = 8; i >= 0; i--) {
            double v = x[i];
            for (int k = i + 1; k < 9; k++) v -= S[9 * k + i] * x[k];
            x[i] = v / S[9 * i + i];
        }
        for (int i = 0; i < 9; i++) Si[9 * i + c] = x[i];
    }
    for (int i = 0; i < 9; i++)   // (the two triangles come from different columns: one value for both)
        for (int j = i + 1; j < 9; j++) Si[9 * i + j] = Si[9 * j + i] = 0.5 * (Si[9 * i + j] + Si[9 * j + i]);
    // W = L^-T Z_b by back-substitution of the border's nine columns (solve_arrow's last loop, nine right-hand sides)
    std::vector<double> W(nc * 9);
    for (size_t ii = nc; ii-- > 0;) {
        const int kmax = (int) std::min<size_t>(BW - 1 - ii % 6, nc - 1 - ii);
        for (int j = 0; j < 9; j++) {
            double v = Z[ii * 10 + j];
            for (int k = 1; k <= kmax; k++) v -= L[(ii + k) * BW + k] * W[(ii + k) * 9 + j];
            W[ii * 9 + j] = v / L[ii * BW];
        }
    }
    // unscale: H = D^-1 Hs D^-1 with D = diag(scale), so H^-1 = D Hs^-1 D
    R.P.assign(9 * nt, 0.0);
    for (int i = 0; i < 9; i++) {
        double *row = &R.P[(size_t) i * nt];
        for (size_t k = 0; k < nc; k++) {
            double v = 0.0;
            for (int j = 0; j < 9; j++) v += Si[9 * i + j] * W[k * 9 + j];
            row[k] = -v * sc[nc + i] * sc[k];
        }
        for (int j = 0; j < 9; j++) R.Sii[9 * i + j] = row[nc + j] = Si[9 * i + j] * (sc[nc + i] * sc[nc + j]);   // (symmetric to the bit)
    }
    R.positive_definite = true;
    return true;
}

// one entry of the solver's chunk table (ecal_solver_chunk_table)
struct ScoreChunk {
    uint32_t cp0, count, seg, span;
};

// cov_robust = G / (G - 1) sum_c s_c s_c^T, s_c = P g_c, g_c = the scores of cluster c's chunks, summed first and scattered into
// the tangent vector (score column i: intrinsic i for i < 9, rotation k of control point cp0 + j at 9 + 3 j + k, translation at
// 21 + 3 j + k).  Cluster id = (seg, (span - 3) / cluster_spans); the chunks are taken in the order of their id, ties in table
// order.  Returns G; cov is written only for G >= 2.
inline uint32_t arrow_cluster_covariance(const IntrinsicsInverse &R, size_t nc, const ScoreChunk *chunks, const double *score, uint32_t n_chunks,
                                         uint32_t cluster_spans, double cov[81]) {
    const size_t nt = nc + 9;
    std::vector<uint32_t> order;
    for (uint32_t c = 0; c < n_chunks; c++)
        if (chunks[c].count && chunks[c].span >= 3 && 6 * ((size_t) chunks[c].cp0 + 4) <= nc) order.push_back(c);
    auto key = [&](uint32_t c) { return ((uint64_t) chunks[c].seg << 32) | (uint64_t) ((chunks[c].span - 3) / cluster_spans); };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    double acc[81];
    for (int i = 0; i < 81; i++) acc[i] = 0.0;
    std::vector<double> g(nt, 0.0);
    uint32_t G = 0;
    for (size_t a = 0; a < order.size();) {
        size_t b = a;
        uint32_t lo = UINT32_MAX, hi = 0;   // the cluster's control points [lo, hi)
        while (b < order.size() && key(order[b]) == key(order[a])) {
            const ScoreChunk &ch = chunks[order[b]];
            const double *sc = score + 33 * (size_t) order[b];
            for (int i = 0; i < 9; i++) g[nc + i] += sc[i];
            for (int j = 0; j < 4; j++)
                for (int k = 0; k < 3; k++) {
                    g[6 * ((size_t) ch.cp0 + j) + k] += sc[9 + 3 * j + k];
                    g[6 * ((size_t) ch.cp0 + j) + 3 + k] += sc[21 + 3 * j + k];
                }
            lo = std::min(lo, ch.cp0);
            hi = std::max(hi, ch.cp0 + 4);
            b++;
        }
        double s[9];
        for (int i = 0; i < 9; i++) {
            const double *row = &R.P[(size_t) i * nt];
            double v = 0.0;
            for (size_t k = 6 * (size_t) lo; k < 6 * (size_t) hi; k++) v += row[k] * g[k];
            for (int j = 0; j < 9; j++) v += row[nc + j] * g[nc + j];
            s[i] = v;
        }
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) acc[9 * i + j] += s[i] * s[j];
        for (size_t k = 6 * (size_t) lo; k < 6 * (size_t) hi; k++) g[k] = 0.0;
        for (int j = 0; j < 9; j++) g[nc + j] = 0.0;
        G++;
        a = b;
    }
    if (G >= 2) {
        const double f = (double) G / (double) (G - 1);
        for (int i = 0; i < 81; i++) cov[i] = f * acc[i];
    }
    return G;
}

// the whole result from the accumulation buffer of one evaluation with Jacobian (accum[0] = the cost) and the chunk scores
inline void arrow_uncertainty(const double *accum, uint32_t n_cp, uint64_t n_res, const ScoreChunk *chunks, const double *score, uint32_t n_chunks,
                              uint32_t cluster_spans, ecal_uncertainty_result *out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    ecal_uncertainty_result &o = *out;
    o = ecal_uncertainty_result{};
    o.n_res = n_res;
    o.n_cp = n_cp;
    o.n_unknowns = 9 + 6 * n_cp;
    o.n_chunks = n_chunks;
    o.cost = accum[0];
    o.s2 = nan;
    for (int i = 0; i < 81; i++) o.cov[i] = o.corr[i] = o.cov_robust[i] = nan;
    for (int i = 0; i < 9; i++) o.sigma[i] = o.sigma_robust[i] = o.inflation[i] = nan;
    ArrowSystem A;
    ArrowWorkspace ws;
    unpack(accum, n_cp, A);
    IntrinsicsInverse R;
    if (!arrow_intrinsics_inverse(A, ws, R)) return;
    o.positive_definite = 1;
    if (n_res > o.n_unknowns) {
        o.formal_valid = 1;
        o.s2 = 2.0 * o.cost / (double) (n_res - o.n_unknowns);
        for (int i = 0; i < 81; i++) o.cov[i] = o.s2 * R.Sii[i];
        for (int i = 0; i < 9; i++) o.sigma[i] = std::sqrt(o.cov[10 * i]);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) o.corr[9 * i + j] = o.cov[9 * i + j] / (o.sigma[i] * o.sigma[j]);
    }
    o.n_clusters = arrow_cluster_covariance(R, A.nc, chunks, score, n_chunks, cluster_spans ? cluster_spans : 1u, o.cov_robust);
    if (o.n_clusters >= 2) {
        o.robust_valid = 1;
        for (int i = 0; i < 9; i++) o.sigma_robust[i] = std::sqrt(o.cov_robust[10 * i]);
        if (o.formal_valid)
            for (int i = 0; i < 9; i++) o.inflation[i] = o.sigma_robust[i] / o.sigma[i];
    }
}
