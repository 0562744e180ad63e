// Counterpart of the reference's EventCalibSpline (continuous-time refinement stage)
//   constructor: gap segmentation, spline initialisation, intrinsics   event_camera_calib/src/EventCalibSpline.cpp:14-113
//   reduceMap (segmentation part)                                      :318-345
//   optimize: event association + Ceres problem                        :115-251
//   updateMap                                                          :253-317
//   SystemBase::saveKeyFrameTrajectoryTUM                              core/system/src/SystemBase.cpp:122-150
// on top of libecal.so: ecal_spline_fit (initial control points), ecal_associate_dev (per-event association on the
// GPU), ecal_solver_* (the Levenberg-Marquardt solve), ecal_spline_eval (poses back at the keyframe times).  The
// map / body-frame object graph of the reference is a plain vector of frames here.
#ifndef ECAL_HOST_EVENT_CALIB_SPLINE_HPP_
#define ECAL_HOST_EVENT_CALIB_SPLINE_HPP_

#include <fstream>
#include <iomanip>

#include "event_calib_ini.hpp"
#include "../../../include/ecal_uncertainty.h"

namespace opengv2 {

class EventCalibSpline {
public:
    struct Frame {
        double timeStamp;
        double twb[3];
        double Qwb[4];                    // x y z w (Eigen coeffs order)
        std::vector<double> circles;      // [n][3] centre x, y, radius in pixels, grid order; NaN rows = erased features
    };
    struct Summary {
        size_t residuals = 0;
        int iterations = 0;
        double initial_cost = 0, final_cost = 0;
    };
    // The calibration quality report (ecal_solver_report) at the solution: the raw residuals, in board units (the unit of
    // Circles_Radius), binned per keyframe of frames(), per circle of the board in grid order, per cell of the sensor and into
    // a histogram.  Filled when the constructor is given report options; valid = false otherwise.
    struct Report {
        bool valid = false;
        ecal_report_options options{};
        ecal_report_totals totals{};
        std::vector<ecal_bin_stats> keyframes, landmarks;
        uint32_t cells_x = 0, cells_y = 0;
        std::vector<uint64_t> cell_n, hist;   // cell_n [cells_y][cells_x]
        std::vector<double> cell_sum_r2;
        double hist_range = 0;                 // the histogram covers [-hist_range, hist_range), its end bins the tails
        static double rms(const ecal_bin_stats &b) { return b.n ? std::sqrt(b.sum_r2 / (double) b.n) : 0.0; }
        double outlierFraction() const { return totals.all.n ? (double) totals.all.n_out / (double) totals.all.n : 0.0; }
        double emptyCellFraction() const {
            size_t empty = 0;
            for (uint64_t n : cell_n) empty += n == 0;
            return cell_n.empty() ? 0.0 : (double) empty / (double) cell_n.size();
        }
    };

    // The same report in PIXELS (ecal_solver_report_px) at the solution: per residual the first-order distance from the event to
    // the projected rim of its circle, binned as above.  Filled when the constructor is given pixel report options; valid = false
    // otherwise.
    struct ReportPx {
        bool valid = false;
        ecal_report_options options{};
        ecal_report_px_totals totals{};
        std::vector<ecal_bin_stats> keyframes, landmarks;
        uint32_t cells_x = 0, cells_y = 0;
        std::vector<uint64_t> cell_n, hist;   // cell_n [cells_y][cells_x]
        std::vector<double> cell_sum_r2;
        double hist_range = 0, outlier_thresh = 0;   // pixels, as the call took them (a value <= 0 in options: the defaults)
        double rmsPx() const { return Report::rms(totals.all); }
        double pxPerUnit() const { return totals.all.n ? totals.sum_px_per_unit / (double) totals.all.n : 0.0; }
        double outlierFraction() const { return totals.all.n ? (double) totals.all.n_out / (double) totals.all.n : 0.0; }
        double emptyCellFraction() const {
            size_t empty = 0;
            for (uint64_t n : cell_n) empty += n == 0;
            return cell_n.empty() ? 0.0 : (double) empty / (double) cell_n.size();
        }
    };

    // The uncertainty of the nine intrinsics (ecal_solver_uncertainty, include/ecal_uncertainty.h) at the solution, on the records the
    // solve ran on: the formal covariance s2 (H^-1)_intr and the cluster-robust one (clusters of clusterSpans knot spans), sigmas,
    // correlations and the ratio of the two sigmas.  Filled when the constructor is given uncertaintyClusterSpans >= 1; valid = false
    // otherwise.  The flags of `result` say which of its parts hold numbers.
    struct Uncertainty {
        bool valid = false;
        uint32_t clusterSpans = 0;
        ecal_uncertainty_result result{};
    };

    // The board-frame event image (ecal_solver_board_image) at the solution: every event of the stream carried through the
    // refined camera and the spline pose at its own time stamp onto the board, with the call's default options (the landmarks'
    // bounding box padded by 3 radii, bin = radius / 8, 64 ring bins over +- radius).  Filled when the constructor is asked for
    // it; valid = false otherwise.
    struct BoardImage {
        bool valid = false;
        ecal_board_image_options options{};
        ecal_board_image_totals totals{};
        std::vector<uint32_t> image;              // [2][height][width]: 0 negative, 1 positive events
        std::vector<ecal_ring_stats> ring_stats;  // [circle][polarity]
        std::vector<uint64_t> ring_hist;          // [circle][ring_bins]
        static double mean(const ecal_ring_stats &r) { return r.n ? r.sum_d / (double) r.n : 0.0; }
        static double stddev(const ecal_ring_stats &r) {
            if (!r.n) return 0.0;
            const double m = mean(r), v = r.sum_d2 / (double) r.n - m * m;
            return v > 0 ? std::sqrt(v) : 0.0;
        }
    };

    // One opt-in refinement round (ecal_solver_create_reassociated): every event of the stream whose board point at the current
    // solution lies within the ring tolerance of a circle's rim becomes a residual, and the solve is repeated from that solution
    // on those records.  refine() has one entry per round; empty unless the constructor is asked for rounds.  Single process.
    struct RefineRound {
        ecal_reassociate_totals totals{};
        size_t residuals = 0;
        int iterations = 0;
        double initial_cost = 0, final_cost = 0;
    };

    // rotation matrix (row-major) -> quaternion xyzw, Eigen::Quaterniond(Matrix3d)'s branch structure
    static void quaternionFromMatrix(const double *m, double *q) {
        double t = m[0] + m[4] + m[8];
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            q[3] = 0.5 * t;
            t = 0.5 / t;
            q[0] = (m[7] - m[5]) * t;
            q[1] = (m[2] - m[6]) * t;
            q[2] = (m[3] - m[1]) * t;
        } else {
            int i = 0;
            if (m[4] > m[0]) i = 1;
            if (m[8] > m[4 * i]) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
            q[i] = 0.5 * t;
            t = 0.5 / t;
            q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
            q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
            q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
        }
    }
    // keyframe pose as the reference stores it (EventCalibIni.cpp:270-278, identity body <- sensor extrinsics)
    static Frame makeFrame(double timeStamp, const EventCalibIni::FramePose &p, const std::vector<CirclesEventFrame::CalibCircle> &features,
                           const std::vector<int> &featureLandmark, size_t n_circles) {
        Frame f;
        f.timeStamp = timeStamp;
        for (int k = 0; k < 3; k++) f.twb[k] = p.twb[k];
        double Rwb[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rwb[3 * i + j] = p.Rsw[3 * j + i];
        quaternionFromMatrix(Rwb, f.Qwb);
        f.circles.assign(3 * n_circles, std::nan(""));
        for (size_t i = 0; i < features.size(); i++) {
            const size_t lm = featureLandmark.empty() ? i : (size_t) featureLandmark[i];
            f.circles[3 * lm] = features[i].location[0];
            f.circles[3 * lm + 1] = features[i].location[1];
            f.circles[3 * lm + 2] = features[i].radius;
        }
        return f;
    }

    EventCalibSpline(std::vector<Frame> frames, EventContainer::Ptr eventContainer, CirclePatternParameters::Ptr pattern, bool useSO3,
                     double motionTimeStep, const double K[4], const double distCoeffs[5], int maxIterations = 50,
                     bool fisheye = false, const ecal_report_options *reportOptions = nullptr, bool wantBoardImage = false,
                     int refineRounds = 0, double refineRingTol = 0.0 /* board units; <= 0: the Huber width */,
                     bool keepEvents = false /* the container's device stream outlives the solve (the caller undistorts it) */,
                     const ecal_report_options *reportPxOptions = nullptr, int uncertaintyClusterSpans = 0 /* >= 1: uncertainty() is filled */)
        : frames_(std::move(frames)), eventContainer_(std::move(eventContainer)), pattern_(std::move(pattern)), useSO3_(useSO3),
          fisheye_(fisheye), motionTimeStep_(motionTimeStep), circleRadius_(pattern_->circleRadius), maxIterations_(maxIterations),
          wantBoardImage_(wantBoardImage), refineRounds_(refineRounds > 0 ? refineRounds : 0), refineRingTol_(refineRingTol),
          keepEvents_(keepEvents) {
        uncertainty_.clusterSpans = uncertaintyClusterSpans > 0 ? (uint32_t) uncertaintyClusterSpans : 0u;
        if (reportOptions) {
            report_.options = *reportOptions;
            wantReport_ = true;
        }
        if (reportPxOptions) {
            reportPx_.options = *reportPxOptions;
            wantReportPx_ = true;
        }
        if (frames_.size() <= 10) throw std::logic_error("too few frames in the map.");  // :26-28
        std::sort(frames_.begin(), frames_.end(), [](const Frame &a, const Frame &b) { return a.timeStamp < b.timeStamp; });
        reduceMap();
        // spline per segment (:61-91)
        segCpOff_.assign(1, 0);
        for (const auto &seg : segments_) {
            std::vector<double> u, tw, qw;
            for (size_t id : seg) {
                u.push_back(frames_[id].timeStamp);
                tw.insert(tw.end(), frames_[id].twb, frames_[id].twb + 3);
                qw.insert(qw.end(), frames_[id].Qwb, frames_[id].Qwb + 4);
            }
            u.front() -= 3 * motionTimeStep_;  // spline can only evaluate inside the bound
            u.back() += 3 * motionTimeStep_;
            time2splineIdx_.emplace_back(u.front(), u.back());
            int cpNum = (int) std::floor((u.back() - u.front()) / (50 * motionTimeStep_));
            if (cpNum > (int) u.size()) cpNum = (int) u.size() - 1;
            if (cpNum < 4) cpNum = 4;  // becomes a Bezier curve
            std::vector<double> kn((size_t) cpNum + 4), ct((size_t) cpNum * 3), cq((size_t) cpNum * 4), kn2((size_t) cpNum + 4);
            int rc = ecal_spline_fit(u.data(), tw.data(), (uint32_t) u.size(), 3, (uint32_t) cpNum, kn.data(), ct.data());
            if (rc == ECAL_OK) rc = ecal_spline_fit(u.data(), qw.data(), (uint32_t) u.size(), 4, (uint32_t) cpNum, kn2.data(), cq.data());
            if (rc != ECAL_OK) throw std::logic_error(std::string("spline initialisation failed: ") + ecal_strerror(rc));
            if (useSO3_) {  // BsplineSO3::initialGuess stores unit quaternions (Sophus::SO3d::setQuaternion) ...
                for (int c = 0; c < cpNum; c++) {
                    double *q = &cq[4 * (size_t) c];
                    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
                    for (int k = 0; k < 4; k++) q[k] /= n;
                }
                // ... and the constructor ends with optimizeCP (BsplineSO3.cpp:55, :285-341): the fit on the group
                rc = ecal_spline_so3_refine(kn2.data(), (uint32_t) cpNum, cq.data(), qw.data(), u.data(), (uint32_t) u.size(), 0, nullptr,
                                            nullptr, nullptr);
                if (rc != ECAL_OK) throw std::logic_error(std::string("SO3 spline refinement failed: ") + ecal_strerror(rc));
            }
            knots_.insert(knots_.end(), kn.begin(), kn.end());
            cpQ_.insert(cpQ_.end(), cq.begin(), cq.end());
            cpT_.insert(cpT_.end(), ct.begin(), ct.end());
            segCpOff_.push_back(segCpOff_.back() + (uint32_t) cpNum);
        }
        // intrinsics (:93-105): only radial distortion (the reference throws for anything else, :97-99).  fisheye (new, BASELINE
        // configs[4]): distCoeffs = cv::fisheye's k1..k4, reverted by the same series into the solver's inverse polynomial
        const double radial[4] = {distCoeffs[0], distCoeffs[1], fisheye_ ? distCoeffs[2] : distCoeffs[4], fisheye_ ? distCoeffs[3] : 0.0};
        double inv[5];
        ecal_inverse_radial_distortion(radial, inv);
        for (int k = 0; k < 4; k++) intrinsics_[k] = K[k];
        for (int k = 0; k < 5; k++) intrinsics_[4 + k] = inv[k];
        optimize();
        updateMap();
    }

    const double *intrinsics() const { return intrinsics_; }  // fx fy cx cy k1..k5 (inverse radial polynomial)
    const std::vector<Frame> &frames() const { return frames_; }
    const Summary &summary() const { return summary_; }
    const Report &report() const { return report_; }
    const ReportPx &reportPx() const { return reportPx_; }
    const Uncertainty &uncertainty() const { return uncertainty_; }
    const BoardImage &boardImage() const { return boardImage_; }
    const std::vector<RefineRound> &refine() const { return refine_; }
    size_t splineNum() const { return segments_.size(); }

    int time2splineIdx(double t) const {
        for (size_t i = 0; i < time2splineIdx_.size(); i++)
            if (t >= time2splineIdx_[i].first && t <= time2splineIdx_[i].second) return (int) i;
        return -1;
    }

    // timestamp tx ty tz qx qy qz qw, one keyframe per line (identity body <- sensor extrinsics: Twc = Twb)
    void saveKeyFrameTrajectoryTUM(const std::string &filename) const {
        std::ofstream f(filename.c_str());
        f << std::fixed;
        for (const auto &bf : frames_)
            f << std::setprecision(10) << bf.timeStamp << " " << bf.twb[0] << " " << bf.twb[1] << " " << bf.twb[2] << " " << bf.Qwb[0]
              << " " << bf.Qwb[1] << " " << bf.Qwb[2] << " " << bf.Qwb[3] << std::endl;
    }

private:
    // :318-345 — a gap of more than 50 steps starts a new spline; segments with fewer than degree + 1 frames are dropped
    void reduceMap() {
        std::vector<std::vector<size_t>> sets(1);
        double last = frames_.front().timeStamp;
        for (size_t i = 0; i < frames_.size(); i++) {
            if (frames_[i].timeStamp - last > 50 * motionTimeStep_) sets.emplace_back();
            sets.back().push_back(i);
            last = frames_[i].timeStamp;
        }
        std::vector<Frame> kept;
        for (auto &s : sets) {
            if (s.size() < 4) continue;
            segments_.emplace_back();
            for (size_t id : s) {
                segments_.back().push_back(kept.size());
                kept.push_back(std::move(frames_[id]));
            }
        }
        frames_ = std::move(kept);
        if (segments_.empty()) throw std::logic_error("sampleSets not filtered");
    }

    bool optimize() {
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const ecal_stream *es = eventContainer_->device();
        const uint64_t n_events = ecal_stream_size(es);
        const uint32_t n_circ = (uint32_t) (pattern_->rows * pattern_->cols), F = (uint32_t) frames_.size();
        std::vector<double> kf_time(F), kf_circ((size_t) F * n_circ * 3);
        for (uint32_t f = 0; f < F; f++) {
            kf_time[f] = frames_[f].timeStamp;
            std::copy(frames_[f].circles.begin(), frames_[f].circles.end(), kf_circ.begin() + (size_t) f * n_circ * 3);
        }
        std::vector<std::array<double, 3>> corners;
        std::vector<double> landmarks;
        for (int i = 0; i < pattern_->rows; i++)
            for (int j = 0; j < pattern_->cols; j++) {
                landmarks.push_back((pattern_->isAsymmetric ? (2 * j + i % 2) : j) * pattern_->squareSize);
                landmarks.push_back(i * pattern_->squareSize);
                landmarks.push_back(0.0);
            }
        ecal_spline_problem prob;
        prob.n_segments = (uint32_t) segments_.size();
        prob.seg_cp_off = segCpOff_.data();
        prob.knots = knots_.data();
        prob.n_res = 0;          // the residual arrays are made on the device (below)
        prob.obs = nullptr;
        prob.time = nullptr;
        prob.lm_id = nullptr;
        prob.seg_id = nullptr;
        prob.n_landmarks = n_circ;
        prob.landmarks = landmarks.data();
        prob.circle_radius = circleRadius_;
        prob.huber_a = 0.2 * circleRadius_;  // :205
        prob.use_so3 = useSO3_ ? 1 : 0;
        prob.camera_model = fisheye_ ? ECAL_CAMERA_FISHEYE : ECAL_CAMERA_RADIAL;
        // :158-192 — every event of every spline's range against its nearest keyframe's circles, and the Ceres problem's
        // residual blocks added where they are found (:181-235): one pass over the resident stream, the records stay in HBM
        std::vector<double> ranges;
        for (size_t i = 0; i < segments_.size(); i++) {
            ranges.push_back(time2splineIdx_[i].first);
            ranges.push_back(time2splineIdx_[i].second);
        }
        ecal_solver *solver = nullptr;
        int rc = ecal_solver_create_from_stream(ctx, es, kf_time.data(), kf_circ.data(), F, n_circ, ranges.data(), (uint32_t) segments_.size(),
                                                5 * motionTimeStep_, 5.0, &prob, &solver);
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_solver_create_from_stream: ") + ecal_last_error(ctx));
        (void) n_events;
        const bool keepStream = wantBoardImage_ || refineRounds_ > 0;   // the board image and the refinement read the stream once more
        if (!keepStream && !keepEvents_) eventContainer_->release();  // eventContainer_->container.clear() (:194)
        summary_.residuals = ecal_solver_num_residuals(solver);
        if (summary_.residuals == 0) {
            ecal_solver_destroy(solver);
            if (keepStream) eventContainer_->release();
            return false;
        }
        std::vector<double> x(ecal_solver_param_size(solver));
        std::copy(intrinsics_, intrinsics_ + 9, x.begin());
        std::copy(cpQ_.begin(), cpQ_.end(), x.begin() + 9);
        std::copy(cpT_.begin(), cpT_.end(), x.begin() + 9 + cpQ_.size());
        ecal_lm_options opt;
        ecal_lm_default_options(&opt);  // the options of :238-243
        opt.max_num_iterations = maxIterations_;
        ecal_lm_summary sm;
        rc = ecal_solver_solve(solver, x.data(), &opt, &sm);
        // opt-in: look at ALL events through the solution, solve on the ones that fit (the reference's TODO at :192)
        for (int round = 0; rc == ECAL_OK && round < refineRounds_; round++) {
            RefineRound r;
            ecal_solver *next = nullptr;
            rc = ecal_solver_create_reassociated(solver, x.data(), es, refineRingTol_, &next, &r.totals);
            if (rc != ECAL_OK) {
                ecal_solver_destroy(solver);
                eventContainer_->release();
                throw std::runtime_error(std::string("ecal_solver_create_reassociated: ") + ecal_last_error(ctx));
            }
            ecal_solver_destroy(solver);
            solver = next;
            r.residuals = ecal_solver_num_residuals(solver);
            if (r.residuals == 0) {
                ecal_solver_destroy(solver);
                eventContainer_->release();
                throw std::runtime_error("refine round: no event within the ring tolerance");
            }
            ecal_lm_summary rs;
            rc = ecal_solver_solve(solver, x.data(), &opt, &rs);
            r.iterations = rs.iterations;
            r.initial_cost = rs.initial_cost;
            r.final_cost = rs.final_cost;
            refine_.push_back(r);
        }
        if (rc == ECAL_OK && wantReport_) {   // at the solution, on the records the solve ran on
            Report &r = report_;
            const ecal_report_options &o = r.options;
            r.cells_x = o.cell_px ? (o.width + o.cell_px - 1) / o.cell_px : 0;
            r.cells_y = o.cell_px ? (o.height + o.cell_px - 1) / o.cell_px : 0;
            r.keyframes.assign(F, ecal_bin_stats{});
            r.landmarks.assign(n_circ, ecal_bin_stats{});
            r.cell_n.assign((size_t) r.cells_x * r.cells_y, 0);
            r.cell_sum_r2.assign(r.cell_n.size(), 0.0);
            r.hist.assign(o.hist_bins, 0);
            r.hist_range = o.hist_range > 0 ? o.hist_range : 4.0 * prob.huber_a;
            rc = ecal_solver_report(solver, x.data(), kf_time.data(), F, &o, &r.totals, r.keyframes.data(), r.landmarks.data(),
                                    r.cell_n.data(), r.cell_sum_r2.data(), r.hist.data());
            r.valid = rc == ECAL_OK;
            if (rc != ECAL_OK) {
                ecal_solver_destroy(solver);
                if (keepStream) eventContainer_->release();
                throw std::runtime_error(std::string("ecal_solver_report: ") + ecal_last_error(ctx));
            }
        }
        if (rc == ECAL_OK && wantReportPx_) {   // the same records, in pixels
            ReportPx &r = reportPx_;
            const ecal_report_options &o = r.options;
            ecal_report_options def;
            ecal_report_px_default_options(&def);
            r.cells_x = o.cell_px ? (o.width + o.cell_px - 1) / o.cell_px : 0;
            r.cells_y = o.cell_px ? (o.height + o.cell_px - 1) / o.cell_px : 0;
            r.keyframes.assign(F, ecal_bin_stats{});
            r.landmarks.assign(n_circ, ecal_bin_stats{});
            r.cell_n.assign((size_t) r.cells_x * r.cells_y, 0);
            r.cell_sum_r2.assign(r.cell_n.size(), 0.0);
            r.hist.assign(o.hist_bins, 0);
            r.hist_range = o.hist_range > 0 ? o.hist_range : def.hist_range;
            r.outlier_thresh = o.outlier_thresh > 0 ? o.outlier_thresh : def.outlier_thresh;
            rc = ecal_solver_report_px(solver, x.data(), kf_time.data(), F, &o, &r.totals, r.keyframes.data(), r.landmarks.data(),
                                       r.cell_n.data(), r.cell_sum_r2.data(), r.hist.data());
            r.valid = rc == ECAL_OK;
            if (rc != ECAL_OK) {
                ecal_solver_destroy(solver);
                if (keepStream) eventContainer_->release();
                throw std::runtime_error(std::string("ecal_solver_report_px: ") + ecal_last_error(ctx));
            }
        }
        if (rc == ECAL_OK && uncertainty_.clusterSpans) {   // the same records: how well they determine the intrinsics
            ecal_uncertainty_options uo;
            ecal_uncertainty_default_options(&uo);
            uo.cluster_spans = uncertainty_.clusterSpans;
            rc = ecal_solver_uncertainty(solver, x.data(), &uo, &uncertainty_.result);
            uncertainty_.valid = rc == ECAL_OK;
            if (rc != ECAL_OK) {
                ecal_solver_destroy(solver);
                if (keepStream) eventContainer_->release();
                throw std::runtime_error(std::string("ecal_solver_uncertainty: ") + ecal_last_error(ctx));
            }
        }
        if (rc == ECAL_OK && wantBoardImage_) {   // every event of the stream through the solution
            BoardImage &b = boardImage_;
            (void) ecal_board_image_default_options(solver, &b.options);
            b.image.assign(2 * (size_t) b.options.width * b.options.height, 0u);
            b.ring_stats.assign(2 * (size_t) n_circ, ecal_ring_stats{});
            b.ring_hist.assign((size_t) n_circ * b.options.ring_bins, 0);
            rc = ecal_solver_board_image(solver, x.data(), es, &b.options, b.image.data(), &b.totals, b.ring_stats.data(), b.ring_hist.data());
            b.valid = rc == ECAL_OK;
            if (rc != ECAL_OK) {
                ecal_solver_destroy(solver);
                eventContainer_->release();
                throw std::runtime_error(std::string("ecal_solver_board_image: ") + ecal_last_error(ctx));
            }
        }
        if (keepStream && !keepEvents_) eventContainer_->release();
        ecal_solver_destroy(solver);
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_solver_solve: ") + ecal_last_error(ctx));
        std::copy(x.begin(), x.begin() + 9, intrinsics_);
        std::copy(x.begin() + 9, x.begin() + 9 + cpQ_.size(), cpQ_.begin());
        std::copy(x.begin() + 9 + cpQ_.size(), x.end(), cpT_.begin());
        summary_.iterations = sm.iterations;
        summary_.initial_cost = sm.initial_cost;
        summary_.final_cost = sm.final_cost;
        return true;
    }

    // :253-317 — keyframe poses re-read from the optimised splines (quaternion variant: blend + normalise; the SO3
    // variant's cumulative evaluation differs from the blend by O(curvature^2) between keyframes and is not replayed here)
    void updateMap() {
        for (auto &bf : frames_) {
            const int idx = time2splineIdx(bf.timeStamp);
            if (idx < 0) continue;
            const uint32_t n_cp = segCpOff_[idx + 1] - segCpOff_[idx];
            const double *kn = &knots_[segCpOff_[idx] + 4 * (size_t) idx];
            double t[3], q[4];
            if (ecal_spline_eval(kn, &cpT_[3 * (size_t) segCpOff_[idx]], n_cp, 3, &bf.timeStamp, 1, t) != ECAL_OK) continue;
            if (ecal_spline_eval(kn, &cpQ_[4 * (size_t) segCpOff_[idx]], n_cp, 4, &bf.timeStamp, 1, q) != ECAL_OK) continue;
            const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            for (int k = 0; k < 3; k++) bf.twb[k] = t[k];
            for (int k = 0; k < 4; k++) bf.Qwb[k] = q[k] / n;
        }
    }

    std::vector<Frame> frames_;
    EventContainer::Ptr eventContainer_;
    CirclePatternParameters::Ptr pattern_;
    bool useSO3_, fisheye_;
    double motionTimeStep_, circleRadius_;
    int maxIterations_;
    std::vector<std::vector<size_t>> segments_;             // sampleIdSets_
    std::vector<std::pair<double, double>> time2splineIdx_;
    std::vector<uint32_t> segCpOff_;
    std::vector<double> knots_, cpQ_, cpT_;
    double intrinsics_[9];
    Summary summary_;
    Report report_;
    bool wantReport_ = false;
    ReportPx reportPx_;
    bool wantReportPx_ = false;
    Uncertainty uncertainty_;
    BoardImage boardImage_;
    bool wantBoardImage_ = false;
    int refineRounds_ = 0;
    double refineRingTol_ = 0.0;
    bool keepEvents_ = false;
    std::vector<RefineRound> refine_;
};

}  // namespace opengv2

#endif  // ECAL_HOST_EVENT_CALIB_SPLINE_HPP_
