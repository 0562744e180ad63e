/*
 * ecal_uncertainty.h — uncertainty of the solved intrinsics (libecal.so, the same library as ecal.h; ABI version unchanged).
 *
 * Three things, all opt-in (nothing in ecal.h calls them):
 *   1. per-chunk score sums: sum over a chunk's records of rho' r J, the gradient of the robust cost split by chunk — what a
 *      cluster-robust covariance needs and neither ecal_solver_evaluate (the total only) nor ecal_residuals (33 doubles a
 *      residual) provides;
 *   2. ecal_solver_uncertainty: the formal covariance s^2 (H^-1)_intr and the cluster-robust (sandwich) covariance of the nine
 *      intrinsics at a parameter vector, with standard deviations, correlations and the ratio of the two sigmas;
 *   3. the sigma map: for one camera and one 9 x 9 covariance, how uncertain the bearing of every sensor pixel is, in pixels.
 * design/24_uncertainty.md has the estimators, their assumptions and what is not known about them.
 *
 * Conventions as in ecal.h: ECAL_OK or a negative ecal_status, _dev = device pointers on `stream`, the others host pointers on
 * the context's stream.  The calls are rank-local and single-process, like ecal_solver_reassociate.
 */
#ifndef ECAL_UNCERTAINTY_H_
#define ECAL_UNCERTAINTY_H_

#include "ecal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-chunk score sums -----------------------------------------------------------------------------------------------------
 * The solver's residual records are cut into chunks (ecal_solver_num_chunks): runs of at most 16384 records inside one knot span
 * of one segment, so that all rows of a chunk share their 33 columns.  For chunk c
 *   score[c][i]  = sum over the chunk's records of (sqrt(rho') r) * (sqrt(rho') J[i]),   i < 33
 *   half_rho[c]  = sum of rho / 2
 * with r, J and the Huber loss exactly as the normal equations see them; column order of ecal_residuals' J: intrinsics 9, rotation
 * tangent of control points cp0 .. cp0 + 3 (3 each), translation of the same four (3 each).  One workgroup per chunk, every thread
 * adds its records in record order, the workgroup's sum is taken in a fixed order without atomics: two calls on the same inputs
 * give the same bits.  A solver without residuals has no chunks: ECAL_OK, nothing is launched or written.
 *   d_score [n_chunks][33], d_half_rho [n_chunks] (NULL: not wanted). */
int ecal_solver_chunk_scores_dev(ecal_solver *s, const double *d_params, double *d_score, double *d_half_rho, void *stream);
int ecal_solver_chunk_scores(ecal_solver *s, const double *params, double *score, double *half_rho);
/* out [n_chunks][4] = (cp0, count, seg, span) of every chunk: cp0 the global index of the first of the chunk's four control points
 * (seg_cp_off[seg] + span - 3), count its records, seg its segment, span its knot span within the segment (>= 3) */
int ecal_solver_chunk_table(ecal_solver *s, uint32_t *out);

/* ---- covariance of the intrinsics ---------------------------------------------------------------------------------------------
 * At `params` (normally the solution): H = the Huber-corrected Gauss-Newton matrix of ecal_solver_evaluate(with_jacobian = 1),
 * n_unknowns = 9 + 6 n_cp, Sigma_ii = (H^-1)[intr, intr] (the inverse of the 9 x 9 Schur complement; no LM diagonal).
 *   formal:  s2 = 2 cost / (n_res - n_unknowns),  cov = s2 Sigma_ii.  Assumes n_res independent residuals of equal variance.
 *   robust:  clusters = the residuals of cluster_spans consecutive knot spans of one segment, id (seg, (span - 3) / cluster_spans);
 *            g_c = the summed score of cluster c in the full tangent vector, s_c = (H^-1)[intr, :] g_c,
 *            cov_robust = G / (G - 1) sum_c s_c s_c^T over the G clusters that hold records.  Assumes independence BETWEEN
 *            clusters only.
 * sigma = sqrt(diag), corr[i][j] = cov[i][j] / (sigma[i] sigma[j]) (of the formal covariance), inflation = sigma_robust / sigma.
 * H not positive definite (a control point without residuals, ...): positive_definite = 0 and every floating-point member except
 * cost is NaN; the call is still ECAL_OK.  n_res <= n_unknowns: formal_valid = 0, s2 / cov / sigma / corr / inflation NaN.
 * G < 2: robust_valid = 0, cov_robust / sigma_robust / inflation NaN.  Order of the nine: fx fy cx cy k1..k5. */
typedef struct ecal_uncertainty_options {
    uint32_t cluster_spans; /* >= 1; default 1 */
    uint32_t reserved;      /* 0 */
} ecal_uncertainty_options;

typedef struct ecal_uncertainty_result {
    uint64_t n_res;
    uint32_t n_unknowns, n_cp, n_chunks, n_clusters;
    uint32_t positive_definite, formal_valid, robust_valid, reserved;
    double cost, s2;
    double cov[81], sigma[9], corr[81];
    double cov_robust[81], sigma_robust[9], inflation[9];
} ecal_uncertainty_result;

void ecal_uncertainty_default_options(ecal_uncertainty_options *o);
int ecal_solver_uncertainty(ecal_solver *s, const double *params, const ecal_uncertainty_options *opt, ecal_uncertainty_result *out);

/* ---- sigma map ----------------------------------------------------------------------------------------------------------------
 * The solver's camera maps a pixel to a ray: x = (u - cx) / fx, y = (v - cy) / fy, rho = x^2 + y^2, (X, Y) = (x, y) g(rho).
 *   ECAL_CAMERA_RADIAL:  g = 1 + k1 rho + .. + k5 rho^5,   g' = k1 + 2 k2 rho + .. + 5 k5 rho^4,   dg/dk_i = rho^i
 *   ECAL_CAMERA_FISHEYE: theta_d = sqrt(rho), theta = theta_d P(rho) with P the same polynomial, g = tan(theta) / theta_d,
 *                        g' = (sec^2(theta) (P / 2 + rho P') - g / 2) / rho,   dg/dk_i = sec^2(theta) rho^i;
 *                        for rho <= 1e-16: g = P and for rho <= 1e-8: g' = P' + P^3 / 3 (the limits at rho -> 0).
 * J (2 x 9) = d (X, Y) / d (fx fy cx cy k1..k5), analytic; E = diag(fx, fy) J is the same in pixels of the ideal camera with the
 * same focal lengths; C = E cov E^T (2 x 2) and sigma_px = sqrt(larger eigenvalue of C), closed form.
 * A pixel that ecal_undistort_points calls invalid (RADIAL: g <= 0; FISHEYE: theta outside [0, pi / 2); a non-finite ray) has
 * flag 1 and sigma_px 0, else flag 0.  Pixel (col, row) is u = col, v = row.  sigma_px [height][width] f64, flag [height][width]
 * u8 (NULL: not wanted).  1 <= width, height <= 8192; fx, fy finite and > 0; else ECAL_ERR_INVALID.  RADIAL: host and device
 * agree bit for bit; FISHEYE: up to tan of the two libraries.
 * intr9 and cov81 are HOST pointers in both calls (ecal_uncertainty_map_dev copies them into its launch arguments: an exception to
 * the "_dev takes device pointers" rule); only d_sigma_px and d_flag are device pointers.
 * ecal_uncertainty_map_host needs no context and no device.  jac (may be NULL) [height][width][18]: J row-major, 0 where invalid. */
int ecal_uncertainty_map_host(int camera_model, const double *intr9, const double *cov81, uint32_t width, uint32_t height,
                              double *sigma_px, uint8_t *flag, double *jac);
int ecal_uncertainty_map_dev(ecal_ctx *ctx, int camera_model, const double *intr9, const double *cov81, uint32_t width, uint32_t height,
                             double *d_sigma_px, uint8_t *d_flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ECAL_UNCERTAINTY_H_ */
