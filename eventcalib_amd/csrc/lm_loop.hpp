// The Levenberg-Marquardt loop of ecal_solver_solve (the Ceres 1.x trust-region minimiser restated) without its device: the trust
// region, what a rank owns in the sharded solves, the seam to whatever evaluates the normal equations (LmDevice: the HIP back end in
// ecal_solver.hip, host threads in tests/cpp/check_lm_loop.cpp) and the loop itself.  Plain C++ — no HIP in here.  Included where
// arrow_host.hpp is, after it (same anonymous namespace, same file-scope includes) and after "ecal.h" and "spline_residual.hpp".
#pragma once
// x (+) delta: intrinsics and translations add, quaternions take exp(delta) (x) q
void plus(const double *x, const std::vector<double> &d, uint32_t n_cp, bool so3, double *out, uint32_t c_lo = 0, uint32_t c_hi = 0xFFFFFFFFu) {
    const size_t nc = 6 * (size_t) n_cp;
    if (c_lo == 0)
        for (int i = 0; i < 9; i++) out[i] = x[i] + d[nc + i];
    for (uint32_t c = c_lo; c < std::min(c_hi, n_cp); c++) {
        if (so3)
            so3_plus(x + 9 + 4 * (size_t) c, &d[6 * (size_t) c], out + 9 + 4 * (size_t) c);
        else
            quaternion_plus(x + 9 + 4 * (size_t) c, &d[6 * (size_t) c], out + 9 + 4 * (size_t) c);
        for (int k = 0; k < 3; k++)
            out[9 + 4 * (size_t) n_cp + 3 * (size_t) c + k] = x[9 + 4 * (size_t) n_cp + 3 * (size_t) c + k] + d[6 * (size_t) c + 3 + k];
    }
}

inline std::chrono::steady_clock::time_point lm_now() { return std::chrono::steady_clock::now(); }
inline double lm_secs(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
struct TrustRegion {
    double radius, decrease_factor = 2.0;
    void reject() { radius /= decrease_factor, decrease_factor *= 2.0; }   // an invalid or a rejected step: shrink the region, faster every time in a row
    void accept(double rel, double max_radius) {
        const double t = 2.0 * rel - 1.0;
        radius = std::min(max_radius, radius / std::max(1.0 / 3.0, 1.0 - t * t * t));
        decrease_factor = 2.0;
    }
};

// What a rank owns (ecal_lm_options.distributed with an all-reduce; ecal.h says what is exchanged when).  mode 1, distributed segments:
// every rank owns its own spline segments in its own ecal_solver; only the 9 intrinsics are shared.  mode 2, time shards of ONE spline
// (SURVEY 8e row 2): every rank holds the whole spline layout and the residuals of its time range — the control points cut into `world`
// interiors with 3-control-point separators (arrow_partition; ecal_solver_time_shard_cuts gives the caller the cut times); every rank
// factorises its own interior, solves the small reduced system redundantly and back-substitutes its own control points.  Nothing
// proportional to the number of control points crosses the links until the solution is put together at the end (gather_part).
struct RankShare {
    int mode = 0, world = 1, rank = 0;        // mode 0: this rank alone (or whole buffers summed: distributed == 0)
    std::vector<uint32_t> ts_first, ts_num;   // mode 2: interiors (control points) of the time shards
    // this rank contributes the unknowns every rank holds the same values for: the intrinsics, the time shards' separators
    bool shared() const { return rank == 0; }
    // the control points whose sums this rank contributes: all of its own; time shards: its interior, with shared() the separators
    template <class F> void each_cp(uint32_t n_cp, F &&f) const {
        const uint32_t lo = mode == 2 ? ts_first[rank] : 0, hi = mode == 2 ? lo + ts_num[rank] : n_cp;
        for (uint32_t c = lo; c < hi; c++) f(c);
        for (int q = 0; mode == 2 && shared() && q + 1 < world; q++)
            for (uint32_t c = ts_first[q] + ts_num[q]; c < ts_first[q] + ts_num[q] + 3; c++) f(c);
    }
    // time shards, the solution put together: every rank contributes its interior, rank 0 the separators and the intrinsics;
    // summed over the ranks `mine` is the whole x (the one exchange proportional to the spline's length, once per solve)
    std::vector<double> gather_part(const std::vector<double> &x, uint32_t n_cp) const {
        std::vector<double> mine(x.size(), 0.0);
        each_cp(n_cp, [&](uint32_t c) {
            for (int k = 0; k < 4; k++) mine[9 + 4 * (size_t) c + k] = x[9 + 4 * (size_t) c + k];
            for (int k = 0; k < 3; k++) mine[9 + 4 * (size_t) n_cp + 3 * (size_t) c + k] = x[9 + 4 * (size_t) n_cp + 3 * (size_t) c + k];
        });
        for (int i = 0; i < 9 && shared(); i++) mine[i] = x[i];
        return mine;
    }
};

constexpr size_t TS_G = (size_t) APZ * (APZ + 1) / 2 + 1;   // upper triangle of an interior's Gram block + its flag
// time shards: the interiors' Gram blocks (upper triangles) + a "positive definite" flag, one slot per rank, summed
inline bool ts_gram_exchange(ArrowParts &pt, const RankShare &share, const std::function<bool(double *, size_t)> &reduce) {
    std::vector<double> buf(TS_G * (size_t) share.world, 0.0);
    double *mine = buf.data() + TS_G * (size_t) share.rank;
    const double *G = pt.G.data() + (size_t) share.rank * APZ * APZ;
    bool finite = true;
    for (size_t i = 0, k = 0; i < (size_t) APZ; i++)
        for (size_t j = i; j < (size_t) APZ; j++) finite = std::isfinite(mine[k++] = G[i * APZ + j]) && finite;
    if (!finite)
        for (size_t q = 0; q + 1 < TS_G; q++) mine[q] = 0.0;
    mine[TS_G - 1] = (pt.ok[share.rank] && finite) ? 1.0 : 0.0;
    if (!reduce(buf.data(), buf.size())) return false;
    for (int p = 0; p < share.world; p++) {
        const double *src = buf.data() + TS_G * (size_t) p;
        double *Gp = pt.G.data() + (size_t) p * APZ * APZ;
        for (size_t i = 0, q = 0; i < (size_t) APZ; i++)
            for (size_t j = i; j < (size_t) APZ; j++) Gp[i * APZ + j] = src[q++];
        pt.ok[p] = src[TS_G - 1] == 1.0 ? 1 : 0;
    }
    return true;
}

// One streamed evaluation, as the loop asks for it.  An: the system at x.  factor: also arrow_part_factor of every interior, with
// the LM diagonal of trust-region radius r_fact (ws / parts then hold what arrow_parts_finish needs).  streamed = false: the
// stream failed to deliver (nothing this code can name should make it) and the buffer was fetched and unpacked the plain way,
// nothing factorised.  reduced_ok (with factor): every separator of the reduced system eliminated.
struct LmStreamJob {
    const double *scale;   // the loop's state the host tasks work on
    double *dd_next;
    ArrowWorkspace *ws;
    ArrowParts *parts;
    const double *x = nullptr;   // this evaluation
    ArrowSystem *An = nullptr;
    bool factor = false;
    double r_fact = 0;
    const std::function<void()> *after_launch = nullptr;   // host work of the loop that only has to be done by the time the kernel is
    double cost = 0;   // its results
    bool streamed = false, reduced_ok = false;
};
// The seam to the device: crossed a handful of times per iteration, never per unknown.
struct LmDevice {
    // evaluate at x (9 + 7 n_cp), with or without the normal equations: the rank-reduced accumulation buffer in acc, *cost = acc[0]
    std::function<int(const double *x, int with_jac, double *cost)> evaluate;
    std::function<bool(double *v, size_t n)> reduce;          // sum v[0..n) over the ranks in place (sharded modes only)
    std::function<int(LmStreamJob &)> evaluate_streamed;      // optional (one rank, the multi-part host solve)
    const double *acc = nullptr;                              // host memory, ecal_solver_normal_size doubles
};
struct LmCounters {   // what last_solve and ECAL_TRACE=solver tell beside the summary
    int n_prefactored = 0;
    bool stream_ok = false;   // in: a streamed evaluation is there to be used; out: still in force at the end
    double t_unpack = 0, t_dd = 0, t_fin = 0, t_quad = 0, t_plus = 0, t_book = 0, t_fin_end = 0, t_fin_back = 0;   // the host's share of an iteration, by item
};
// x: in the start, out the last accepted point (time shards: this rank's view of it — RankShare::gather_part).  pool / n_parts: one
// rank, a long spline: the factorisation, the unpacking and the quadratic forms run on several host cores
// (arrow_host_parts.hpp); the sharded modes keep the sequential routines (their segments are short, and the sequential routine's
// 10 x 10 Schur sums are what the ranks exchange; unpacking and the quadratic forms still use the pool).
inline int lm_loop(const LmDevice &dev, const ecal_lm_options &opt, const RankShare &share, uint32_t n_cp, bool use_so3, HostPool *pool, int n_parts,
                   std::vector<double> &x, ecal_lm_summary &S, LmCounters &K) {
    const size_t np = x.size(), nc = 6 * (size_t) n_cp, nt = nc + 9;
    const bool ts_mode = share.mode == 2, dist_mode = share.mode != 0, parts_solve = !dist_mode;
    const int world = share.world, my_rank = share.rank;
    const double *const acc = dev.acc;
    std::vector<double> xc(np), delta, scale(nt, 1.0), dd(nt), dd_next(nt);
    ArrowSystem A, A_next;
    ArrowWorkspace ws;
    ArrowParts parts, ts_parts;
    const std::function<bool(ArrowParts &)> ts_exchange = [&](ArrowParts &pt) -> bool { return ts_gram_exchange(pt, share, dev.reduce); };
    auto unpack_acc = [&]() {
        const auto tu = lm_now();
        if (pool) {   // band rows by ranges of control points, one range per task
            unpack_alloc(n_cp, A);
            unpack_head(acc, A);
            const uint32_t T = 4u * (uint32_t) n_parts, per = (n_cp + T - 1) / T;
            pool->run((int) T, [&](int t) { unpack_rows(acc, A, std::min(n_cp, (uint32_t) t * per), std::min(n_cp, ((uint32_t) t + 1) * per)); });
        } else unpack(acc, n_cp, A);
        K.t_unpack += lm_secs(tu, lm_now());
    };
    // Streamed evaluation (one rank, the multi-part host solve): the kernel delivers the records group by group, the pool's
    // threads unpack an interior's rows and, when the trust-region radius the next linear solve will use can be predicted,
    // factorise it while the kernel is still busy with the later control points.  What is left behind the kernel: the last
    // interior, the separators' rows, the reduced system, the back-substitution.
    bool &stream_ok = K.stream_ok;
    LmStreamJob job{scale.data(), dd_next.data(), &ws, &parts};
    auto evaluate_streamed = [&](const double *xp, ArrowSystem &An, bool factor, double r_fact, const std::function<void()> *after_launch) -> int {
        job.x = xp, job.An = &An, job.factor = factor, job.r_fact = r_fact, job.after_launch = after_launch;
        return dev.evaluate_streamed(job);
    };
    memset(&S, 0, sizeof(S));
    TrustRegion tr{opt.initial_trust_region_radius};
    int rc;
    bool fact_ready = false;      // ws / parts hold the interiors' factors for A with the diagonal of radius fact_radius
    double cost = 0, fact_radius = 0;
    if (stream_ok) {   // (the column scaling comes from this evaluation: nothing to factorise with yet)
        if ((rc = evaluate_streamed(x.data(), A, false, 0.0, nullptr))) return rc;
        cost = job.cost;
        if (!job.streamed) stream_ok = false;
    } else {
        if ((rc = dev.evaluate(x.data(), 1, &cost))) return rc;
        unpack_acc();
    }
    S.jacobian_evaluations = 1, S.initial_cost = cost;
    if (opt.jacobi_scaling) {  // computed once from the initial Jacobian, as Ceres does
        for (size_t i = 0; i < nc; i++) scale[i] = 1.0 / (1.0 + std::sqrt(A.band[i * BW]));
        for (int i = 0; i < 9; i++) scale[nc + i] = 1.0 / (1.0 + std::sqrt(A.corner[10 * i]));
    }
    S.termination = 1;  // NO_CONVERGENCE unless a test fires
    auto gmax = [&]() {
        double m = 0;
        for (size_t i = 0; i < nc; i++) m = std::max(m, std::fabs(A.gc[i]));
        if (dist_mode) {  // one slot per rank, summed: a max over ranks without a max collective
            std::vector<double> v((size_t) world, 0.0);
            v[(size_t) my_rank] = m;
            if (dev.reduce(v.data(), v.size()))
                for (double x : v) m = std::max(m, x);
        }
        for (int i = 0; i < 9; i++) m = std::max(m, std::fabs(A.gi[i]));
        return m;
    };
    if (dist_mode)
        ws.reduce_G = [&](double *G) -> bool {
            double buf[101];
            bool bad = false;
            for (int i = 0; i < 100; i++) bad = bad || !std::isfinite(G[i]);
            for (int i = 0; i < 100; i++) buf[i] = bad ? 0.0 : G[i];
            buf[100] = bad ? 1.0 : 0.0;
            if (!dev.reduce(buf, 101)) return false;
            for (int i = 0; i < 100; i++) G[i] = buf[i];
            return buf[100] == 0.0;
        };
    if (gmax() <= opt.gradient_tolerance) S.termination = 0;
    bool last_step_ok = true;
    auto reject = [&] { tr.reject(), S.unsuccessful_steps++; };
    // the interiors factorised and the separators eliminated while the kernel ran: the intrinsics' corner and the way back
    auto prefactored_finish = [&]() -> bool {
        const auto ta = lm_now();
        if (!job.reduced_ok || !arrow_reduced_end(A, scale.data(), dd.data(), parts)) return false;
        const auto tb = lm_now();
        arrow_parts_backsub(A.nc, delta, ws, parts, pool, n_parts);
        K.t_fin_end += lm_secs(ta, tb), K.t_fin_back += lm_secs(tb, lm_now());
        return true;
    };
    while (S.termination == 1 && S.iterations < opt.max_num_iterations) {
        S.iterations++;
        const auto t_it = lm_now();
        // Levenberg-Marquardt diagonal on the scaled system (the streamed evaluation left the control points' part behind when
        // its radius is the one in force)
        const bool prefactored = fact_ready && fact_radius == tr.radius && job.reduced_ok;
        if (prefactored) memcpy(dd.data(), dd_next.data(), nc * sizeof(double));
        for (size_t i = prefactored ? nc : 0; i < nt; i++) {
            const double h = (i < nc ? A.band[i * BW] : A.corner[10 * (i - nc)]) * scale[i] * scale[i];
            dd[i] = std::min(std::max(h, opt.min_lm_diagonal), opt.max_lm_diagonal) / tr.radius;
        }
        const auto tl = lm_now();
        K.t_dd += lm_secs(t_it, tl);
        bool ok = ts_mode ? solve_arrow_parts(A, scale, dd, delta, ws, ts_parts, nullptr, world, my_rank, &ts_exchange)
                  : (n_parts > 1 && parts_solve)
                      ? (fact_ready && fact_radius == tr.radius ? prefactored_finish()   // (false when an interior or a separator was not positive definite)
                                                                : solve_arrow_parts(A, scale, dd, delta, ws, parts, pool, n_parts))   // (a whole factorisation: the even partition — the streamed evaluation sets up its own)
                      : solve_arrow(A, scale, dd, delta, ws);
        if (fact_ready && fact_radius == tr.radius) K.n_prefactored++;
        fact_ready = false;
        const auto t_q = lm_now();
        K.t_fin += lm_secs(tl, t_q);
        double model_change = 0;
        // After a successful step the next one is usually successful too: evaluate the candidate WITH its normal
        // equations in one pass (4.8 ms) instead of a cost-only pass (1.0 ms + a host round trip) followed, on
        // acceptance, by the full pass at the same point.  After a rejected step fall back to the cost-only probe.
        const bool speculate = last_step_ok;
        // streamed evaluation ahead: the quadratic forms of the model are computed once the kernel is running (they gate the
        // evaluation only when the step is no descent step of the model, which a positive definite system rules out up to rounding)
        const bool defer_quad = ok && !dist_mode && speculate && stream_ok;
        double gTd_late = 0, dHd_late = 0;
        if (defer_quad) {
            for (size_t i = 0; i < nt; i++) delta[i] *= scale[i];
            model_change = 1.0;   // (placeholder until the forms are in)
        } else if (ok && ts_mode) {
            // the step solves (H + D) y = -g exactly, so y^T H y = -g^T y - y^T D y and the model change -g^T y - y^T H y / 2 is
            // (y^T D y - g^T y) / 2: sums over unknowns — this rank's interior, rank 0 also the separators and the intrinsics
            // (every rank holds the same values for those)
            double two[2] = {0, 0};
            auto add = [&](size_t i) {
                const double g = i < nc ? A.gc[i] : A.gi[i - nc];
                two[0] += g * scale[i] * delta[i];
                two[1] += dd[i] * delta[i] * delta[i];
            };
            share.each_cp(n_cp, [&](uint32_t c) { for (size_t i = 6 * (size_t) c; i < 6 * (size_t) c + 6; i++) add(i); });
            for (size_t i = nc; i < nt && share.shared(); i++) add(i);
            if (!dev.reduce(two, 2)) return ECAL_ERR_HIP;
            for (size_t i = 0; i < nt; i++) delta[i] *= scale[i];
            model_change = 0.5 * (two[1] - two[0]);
            ok = model_change > 0.0;
        } else if (ok) {
            for (size_t i = 0; i < nt; i++) delta[i] *= scale[i];
            double two[2];   // g^T d, d^T H d
            quad_forms(A, delta, &two[0], &two[1], dist_mode && !share.shared(), pool, n_parts);
            if (dist_mode && !dev.reduce(two, 2)) return ECAL_ERR_HIP;
            model_change = -two[0] - 0.5 * two[1];
            ok = model_change > 0.0;
        }  // (a failed factorisation was agreed on through reduce_G: every rank skips the reduction above together)
        S.seconds_linear_solve += lm_secs(tl, lm_now()), K.t_quad += lm_secs(t_q, lm_now());
        if (!ok) {  // invalid step: shrink the region
            reject();
            continue;
        }
        const auto t_p = lm_now();
        plus(x.data(), delta, n_cp, use_so3, xc.data());   // (on the pool's threads: measured slower, 47 against 28 us)
        K.t_plus += lm_secs(t_p, lm_now());
        double new_cost;
        // streamed: the interiors are factorised for the radius a step with rel >= 0.937 leads to (the usual one while the
        // model is good: radius / max(1/3, 1 - (2 rel - 1)^3) = radius / (1/3)); any other verdict factorises again as before
        const double r_pred = std::min(opt.max_trust_region_radius, tr.radius / (1.0 / 3.0));
        bool cand_in_next = false, cand_factored = false;   // the candidate's system sits unpacked in A_next / its interiors are factorised
        if (speculate && stream_ok) {
            const std::function<void()> late = [&] { quad_forms(A, delta, &gTd_late, &dHd_late, false, pool, n_parts); };
            rc = evaluate_streamed(xc.data(), A_next, true, r_pred, defer_quad ? &late : nullptr);
            new_cost = job.cost, cand_factored = job.streamed, cand_in_next = true;
            if (!rc && !cand_factored) stream_ok = false;   // (fetched the plain way: carry on without the stream)
        } else {
            rc = dev.evaluate(xc.data(), speculate ? 1 : 0, &new_cost);
        }
        if (rc) return rc;
        const auto t_b = lm_now();
        if (defer_quad) {
            model_change = -gTd_late - 0.5 * dHd_late;
            if (!(model_change > 0.0)) {   // invalid step after all: the evaluation is dropped, the region shrinks
                S.jacobian_evaluations++;
                reject();
                continue;
            }
        }
        if (speculate) S.jacobian_evaluations++; else S.cost_evaluations++;
        const double rel = (cost - new_cost) / model_change;
        double norm2[2] = {0, 0}, &step2 = norm2[0], &x2 = norm2[1];
        if (ts_mode) {   // own interior from every rank; separators and intrinsics once (rank 0)
            share.each_cp(n_cp, [&](uint32_t c) {
                for (int k = 0; k < 6; k++) step2 += delta[6 * (size_t) c + k] * delta[6 * (size_t) c + k];
                for (int k = 0; k < 4; k++) x2 += x[9 + 4 * (size_t) c + k] * x[9 + 4 * (size_t) c + k];
                for (int k = 0; k < 3; k++) x2 += x[9 + 4 * (size_t) n_cp + 3 * (size_t) c + k] * x[9 + 4 * (size_t) n_cp + 3 * (size_t) c + k];
            });
            if (share.shared()) {
                for (size_t i = nc; i < nt; i++) step2 += delta[i] * delta[i];
                for (size_t i = 0; i < 9; i++) x2 += x[i] * x[i];
            }
        } else {   // (distributed segments: own control points from every rank, the shared intrinsics once, after the sum)
            for (size_t i = 0; i < (dist_mode ? nc : nt); i++) step2 += delta[i] * delta[i];
            for (size_t i = dist_mode ? 9 : 0; i < np; i++) x2 += x[i] * x[i];
        }
        if (dist_mode && !dev.reduce(norm2, 2)) return ECAL_ERR_HIP;
        if (dist_mode && !ts_mode) {
            for (size_t i = nc; i < nt; i++) step2 += delta[i] * delta[i];
            for (size_t i = 0; i < 9; i++) x2 += x[i] * x[i];
        }
        if (rel > opt.min_relative_decrease) {
            const double cost_change = cost - new_cost, prev = cost;
            x.swap(xc);
            if (speculate) {
                cost = new_cost;  // the buffer of the speculative pass is the one to unpack
            } else {
                rc = dev.evaluate(x.data(), 1, &cost);
                if (rc) return rc;
                S.jacobian_evaluations++;
            }
            if (cand_in_next) std::swap(A, A_next);   // (unpacked while the kernel ran)
            else unpack_acc();
            S.successful_steps++, last_step_ok = true;
            tr.accept(rel, opt.max_trust_region_radius);
            if (cand_factored) fact_ready = true, fact_radius = r_pred;
            if (gmax() <= opt.gradient_tolerance) S.termination = 0;
            else if (std::fabs(cost_change) <= opt.function_tolerance * prev) S.termination = 0;
        } else {
            reject();
            last_step_ok = false;
        }
        if (S.termination == 1 && std::sqrt(step2) <= opt.parameter_tolerance * (std::sqrt(x2) + opt.parameter_tolerance)) S.termination = 0;
        K.t_book += lm_secs(t_b, lm_now());
    }
    S.final_cost = cost;
    return ECAL_OK;
}
