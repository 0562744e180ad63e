/*
 * ecal.h — C ABI of the MI355X-native EventCalib hot path (libecal.so).
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Every entry point names the reference
 * interface it replaces (paths relative to the reference tree, MobilePerceptionLab/EventCalib).
 * The reference has no FFI layer of its own; its seams are the C++ class APIs listed here, and
 * the C++ shims in eventcalib_amd/csrc/host/ (same class names and members) sit on top of this
 * ABI so that unit_test_eventCameraCalib-style callers can switch with a re-link
 * (INTEGRATION.md shows the binding).
 *
 * Conventions: returns ECAL_OK (0) or a negative ecal_status; never throws; all buffers are
 * caller-owned; outputs are written only on success.  Entry points ending in _dev take DEVICE
 * pointers and enqueue asynchronously on `stream` (a hipStream_t passed as void*; NULL is HIP's
 * default stream, exactly as in a kernel launch); the others take HOST pointers, run on the
 * context's own stream and return when the result is in place.
 * One ecal_ctx per host thread (matches the reference's one-DBSCAN-instance-per-worker use,
 * event_camera_calib/test/eventCameraCalib.cpp:181-190).
 */
#ifndef ECAL_H_
#define ECAL_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECAL_ABI_VERSION 3

typedef enum ecal_status {
    ECAL_OK = 0,
    ECAL_ERR_INVALID = -1,    /* bad argument (NULL pointer, minpts < 1, ...) */
    ECAL_ERR_NO_DEVICE = -2,  /* no usable HIP device / HIP runtime failure at init */
    ECAL_ERR_HIP = -3,        /* a HIP call failed; ecal_last_error() has the text */
    ECAL_ERR_NOMEM = -4,      /* device or host allocation failed */
    ECAL_ERR_UNSORTED = -5,   /* event timestamps are not non-decreasing */
    ECAL_ERR_RANGE = -6,      /* a size exceeds what the ABI can index (2^32-1 points) */
    ECAL_ERR_COMM = -7        /* RCCL error (ecal_last_error has the text) */
} ecal_status;

typedef struct ecal_ctx ecal_ctx;

/* ---- lifecycle -------------------------------------------------------------------------- */
int ecal_abi_version(void);
int ecal_init(int device, ecal_ctx **out);
void ecal_destroy(ecal_ctx *ctx);
const char *ecal_strerror(int status);
const char *ecal_last_error(const ecal_ctx *ctx);
/* blocks until everything enqueued on the context's own stream has finished */
int ecal_sync(ecal_ctx *ctx);

/* ---- DBSCAN ------------------------------------------------------------------------------
 * Replaces DBSCAN<Eigen::Vector2d,double>::Run(&V, 2, eps, minpts)
 *   (dbscan/include/dbscan.h:115-177, regionQuery :198-227, expandCluster :229-259) and the
 *   kd-tree underneath it (dbscan/src/kdtree.cpp:106-179, 344-365), called twice per
 *   time-slice from CirclesEventFrame::extractFeatures (event_camera_calib/src/CirclesEventFrame.cpp:66-72).
 *
 * One Run() per slice s over the points xy[slice_off[s] .. slice_off[s+1]) (pid = index inside
 * the slice, dim = 2).  labels[i] = index into the reference's `Clusters` vector for that slice
 * (clusters are numbered in order of their smallest member pid, dbscan.h:154-155), or -1 for a
 * member of `Noise`.  Only core points (>= minpts neighbours, self excluded, dbscan.h:151,218,247)
 * are ever assigned; border points are Noise exactly as in the reference.  The neighbour
 * relation reproduces the reference kd-tree's inclusive-ball / strict-plane-pruning behaviour
 * bit for bit (DESIGN.md "the quirk").  Empty slices give n_clusters[s] = 0 (Run would return
 * FAILED, dbscan.h:121); minpts < 1 is ECAL_ERR_INVALID (Run's FAILED, dbscan.h:123).
 */
int ecal_dbscan_batch(ecal_ctx *ctx, const double *xy /*[N][2]*/, const uint32_t *slice_off /*[S+1]*/,
                      uint32_t S, double eps, uint32_t minpts, int32_t *labels /*[N]*/,
                      uint32_t *n_clusters /*[S]*/);

/* Device-resident form: segment s is d_xy[d_seg_off[s] .. d_seg_off[s]+d_seg_cnt[s]) (segments
 * may leave gaps but must not overlap); n_points = upper bound on any d_seg_off+d_seg_cnt
 * (size of d_xy/d_labels in points).  max_seg_points: upper bound on any d_seg_cnt, or 0 if
 * unknown (then every size tier is launched). */
int ecal_dbscan_batch_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                          uint32_t S, uint32_t n_points, uint32_t max_seg_points, double eps, uint32_t minpts,
                          int32_t *d_labels, uint32_t *d_n_clusters, void *stream);

/* ecal_cluster_order_dev: the member ORDER of DBSCAN<T,Float>::Clusters (dbscan.h:92): d_order[slot] = position of the
 * point inside Clusters[label] — the order expandCluster's queue pops the cluster's core points in (dbscan.h:229-265; the
 * seed = the cluster's smallest pid first), which follows the result order of the kd-tree's range query (hits in reverse
 * visiting order, kdtree.cpp:148-179,469-486) —, -1 for Noise.  d_xy / d_seg_off / d_seg_cnt as ecal_dbscan_batch_dev
 * takes them, d_labels / d_n_clusters as it returned them, same eps.  d_status[s] = 0, or 1 for a segment this pass does
 * not take (more than 2^20 points, or range-query result lists of more than 2^24 entries in all — segments of up to 4096
 * points run in LDS, anything beyond or denser in a global workspace): its d_order entries are -1.  What it is for: Clusters[c] in the reference's order for callers that index into it, and
 * extractFeatures' medians (std::nth_element over Clusters[c], CirclesEventFrame.cpp:136-147), which depend on that order
 * when two members tie in norm.  only_tied_medians != 0: the order is worked out only for the clusters that need it for that
 * purpose — those whose member of rank size / 2 in the order (norm, pid) shares its norm with another member (the test
 * ecal_extract_batch_ordered_dev applies) —, the members of all other clusters get -2; segments without such a cluster do
 * not even have their tree rebuilt.  (only_tied_medians == 2, used by ecal_extract_batch_exact_dev: the caller has named
 * those clusters itself by storing -3 in d_order on the slot of one member of each.)
 * Four launches: segments of up to 768 points and 256 clusters, then up to 2048 points, then up to 4096, then the rest.
 * Contract on the hand-over of kd-trees: the last ecal_dbscan_batch*_dev call of the context leaves the trees of its first-pass
 * segments behind (4 bytes per point in context scratch); they are replayed here instead of being rebuilt when d_labels,
 * d_seg_off and S are that call's.  Any slicing entry point and ecal_copy_dev on the context drop them; a caller that
 * rewrites the points or labels of those buffers by other means must call ecal_dbscan_batch*_dev again before this. */
int ecal_cluster_order_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, uint32_t S,
                           double eps, const int32_t *d_labels, const uint32_t *d_n_clusters, int32_t *d_order /*[n_points]*/,
                           uint32_t *d_status /*[S]*/, int only_tied_medians, void *stream);
/* host-buffer form (what host/dbscan.h calls): slices as ecal_dbscan_batch takes them, labels / n_clusters as it returned them */
int ecal_cluster_order(ecal_ctx *ctx, const double *xy, const uint32_t *slice_off /*[S+1]*/, uint32_t S, double eps,
                       const int32_t *labels, const uint32_t *n_clusters /*[S]*/, int32_t *order /*[N]*/, uint32_t *status /*[S]*/);

/* ---- ingest + time-slicing ----------------------------------------------------------------
 * The event stream is the reference's .bin image: packed 25-byte little-endian records
 * {f64 t_sec, f64 x, f64 y, u8 polarity} (event/include/opengv2/event/Event.hpp:41-47,
 * README.md:7-13), time-sorted as the reference's std::multimap<double,Event_loc_pol> keeps them
 * (event_camera_calib/test/eventCameraCalib.cpp:154-163).  At most 2^32-1 events per stream.
 *
 * ecal_window_bounds_dev: for every window s the index range [lo, hi) of the events with
 *   t0[s] <= t <= t1[s] — container.lower_bound(duration.first) .. upper_bound(duration.second)
 *   of EventFrame::EventFrame (event/src/EventFrame.cpp:14-15) — and win_base[s] = sum of the
 *   sizes of the windows before s (win_base[S] = total), the slot where window s writes.
 * ecal_check_sorted_dev: *d_flag = 1 if some timestamp is smaller than its predecessor.
 * ecal_slice_events_dev: the rest of the EventFrame constructor (EventFrame.cpp:10-36) for all
 *   windows at once: per polarity the set of unique pixel locations (operator== on the doubles),
 *   minus every location present in both sets.  Window s owns slots [win_base[s], win_base[s+1])
 *   of d_xy / d_event_point (capacity cap_points slots):
 *     segment 2s   = positiveEvents_ : d_xy[d_seg_off[2s]   ..+d_seg_cnt[2s]]
 *     segment 2s+1 = negativeEvents_ : d_xy[d_seg_off[2s+1] ..+d_seg_cnt[2s+1]]
 *   in the element order ecal_set_point_order selected: by default THE REFERENCE'S — the iteration
 *   order of its std::unordered_set<Vector2d, EigenMatrixHash> (EventFrame.cpp:12-13,34-35;
 *   core/utility/include/opengv2/utility/utility.hpp:38-51; libstdc++), which DBSCAN's cluster
 *   assignments depend on (insertion-order kd-tree, kdtree.cpp:128-131,169) — or first occurrence.
 *   d_event_point[win_base[s]+k] = index of event k's pixel inside its polarity's segment, or -1
 *   if the pixel was erased — an output of this library's own (the reference's EventFrame keeps no such map; the
 *   association stage uses it); d_event_point == NULL: not wanted, not written (4 bytes per event less to write,
 *   one table phase less in the slicer).  The segment arrays feed ecal_dbscan_batch_dev directly (S' = 2S).
 *   *d_overflow = 1 if some window did not fit cap_points (its segments are then empty).
 *   max_win_events: upper bound on any window size, 0 = unknown.
 */
/* Element order of the pixel sets every slicing entry point of this context emits (ecal_slice_events_dev and everything
 * built on it: ecal_detect_fused_dev, ecal_detect_batch, ecal_detect_pass, ecal_detect_keyframes, ecal_detect_stream_tiled).  ECAL_ORDER_REFERENCE (default): positiveEvents_ / negativeEvents_ exactly
 * as the reference's EventFrame constructor leaves them on libstdc++ — same `.bin` => same point order => same DBSCAN
 * labels as the reference.  ECAL_ORDER_FIRST_OCCURRENCE: ascending first occurrence of the pixel inside the window (the
 * same sets, a cheaper order; labels then equal the reference's only up to the order-dependent effects). */
enum { ECAL_ORDER_REFERENCE = 0, ECAL_ORDER_FIRST_OCCURRENCE = 1 };
int ecal_set_point_order(ecal_ctx *ctx, int order);
int ecal_get_point_order(const ecal_ctx *ctx);
/* the restated libstdc++ tables behind ECAL_ORDER_REFERENCE, exported for verification (no GPU needed): bucket count of
 * epoch e (13, 29, 59, ...; 0 past the table) and EigenMatrixHash of a pixel */
uint64_t ecal_ref_bucket_step(int epoch);
uint64_t ecal_ref_pixel_hash(double x, double y);

/* (One stream per context runs the single-launch form — the first stream that calls; calls on other streams of the same
 * context are correct too but take two launches: the look-back table of the fused scan is context scratch.) */
int ecal_window_bounds_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const double *d_t0,
                           const double *d_t1, uint32_t S, uint32_t *d_win_lo, uint32_t *d_win_hi,
                           uint32_t *d_win_base /*[S+1]*/, void *stream);
int ecal_check_sorted_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, int *d_flag, void *stream);
/* d_sorted (n_events * 25 bytes, not overlapping d_events) = the records in the order the reference's
 * std::multimap<double, Event_loc_pol> iterates in (eventCameraCalib.cpp:154-163): ascending time stamp, records with
 * equal time stamps in their input order (stable).  For streams that do not arrive in time order; the _dev entry points
 * above take time-ordered records, ecal_stream_create sorts by itself when it has to. */
int ecal_sort_events_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, uint8_t *d_sorted, void *stream);
int ecal_slice_events_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const uint32_t *d_win_lo,
                          const uint32_t *d_win_hi, const uint32_t *d_win_base, uint32_t S, uint32_t max_win_events,
                          uint32_t cap_points, double *d_xy, uint32_t *d_seg_off /*[2S]*/,
                          uint32_t *d_seg_cnt /*[2S]*/, int32_t *d_event_point, int *d_overflow, void *stream);

/* ---- packed points -----------------------------------------------------------------------------------------------------
 * Event pixels are small integers: between the stages a point needs 4 bytes (x | y << 16, two's complement int16 each), not
 * the 16 of the reference's Vector2d.  The *_packed_dev forms of the three stage entry points take an ecal_packed_points
 * (caller-owned device buffers: d_xy16 [cap_points], d_seg_fmt [2S]; NULL = the plain forms): the slicer writes the windows
 * its pixel kernels take (sensor pixels 0 <= x <= 2047, 0 <= y <= 1023, up to 2047 events; x <= 1023 up to 4095 events; in
 * reference order x <= 511 up to 5119 events) to d_xy16 only and marks their two
 * segments d_seg_fmt = 1; every other window goes to d_xy as doubles (d_seg_fmt = 0).  DBSCAN and the extraction read
 * whichever form a segment has (and write its doubles themselves, d_seg_fmt 1 -> 3, before a segment goes to one of their
 * general tiers); results are bit for bit those of the plain forms.  ecal_unpack_points_dev writes the doubles of every
 * segment that has none yet — for callers that want d_xy itself (positiveEvents_ / negativeEvents_ as doubles). */
typedef struct ecal_packed_points {
    uint32_t *d_xy16;     /* [cap_points] */
    uint32_t *d_seg_fmt;  /* [2S]: 0 doubles only, 1 packed only, 3 both */
} ecal_packed_points;
int ecal_slice_events_packed_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const uint32_t *d_win_lo,
                                 const uint32_t *d_win_hi, const uint32_t *d_win_base, uint32_t S, uint32_t max_win_events,
                                 uint32_t cap_points, double *d_xy, uint32_t *d_seg_off, uint32_t *d_seg_cnt, int32_t *d_event_point,
                                 int *d_overflow, const ecal_packed_points *pk, void *stream);
int ecal_dbscan_batch_packed_dev(ecal_ctx *ctx, double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, uint32_t S,
                                 uint32_t n_points, uint32_t max_seg_points, double eps, uint32_t minpts, int32_t *d_labels,
                                 uint32_t *d_n_clusters, const ecal_packed_points *pk, void *stream);
/* (the extraction the context's ecal_set_median_ties setting asks for: ecal_extract_batch_exact_dev or ecal_extract_batch_dev) */
int ecal_extract_batch_packed_dev(ecal_ctx *ctx, double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                                  const int32_t *d_labels, const uint32_t *d_n_clusters, uint32_t S /*windows*/, uint32_t n_points,
                                  double eps, uint32_t cluster_min, uint32_t need_clusters, double radius_threshold, int fit_circle,
                                  uint32_t knn_num, uint32_t *d_win_info, uint32_t *d_cand_pair, double *d_cand_xyr,
                                  int32_t *d_kept_labels, uint32_t *d_rep, const ecal_packed_points *pk, void *stream);
int ecal_unpack_points_dev(ecal_ctx *ctx, const ecal_packed_points *pk, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                           uint32_t n_segments, double *d_xy, void *stream);

/* ---- circle-candidate extraction -----------------------------------------------------------
 * Replaces CirclesEventFrame::extractFeatures between its DBSCAN::Run calls and cv::findCirclesGrid
 * (event_camera_calib/src/CirclesEventFrame.cpp:89-312) for all windows at once: fit_circle == 0 is the
 * mutual-nearest / midpoint path of :283-311 (the shipped example.yaml), fit_circle != 0 the knn_num-nearest
 * / algebraic CirclesEventFrame::fitCircle (:361-415) / double-direction path of :180-281 (knn_num <= 8).  Inputs are the outputs of ecal_slice_events_dev and ecal_dbscan_batch_dev with
 * S' = 2S segments (2s = positive, 2s+1 = negative polarity of window s).
 * knn_num (fit_circle != 0, 1..8): the neighbour list of a representative holds its knn_num nearest representatives of the
 *   other polarity in ascending squared distance, equal distances in ascending cluster index.  With FEWER kept clusters of
 *   that polarity than knn_num the list ENDS at their number — each cluster appears once — and the two gates of :187-193
 *   (d > 4 d0, d > 4 radius_threshold^2; a neighbour AT either bound stays) then cut it as usual.  (The reference there reads
 *   on into whatever its reused result vectors held, :173-193 and :232-241; design/04_slicing_extraction.md, section 4f.)
 *
 * ecal_circle_radius_threshold: circleRadiusThreshold_ (CirclesEventFrame.cpp:16-33); pure host math.
 * ecal_extract_batch_dev, per window s (all outputs indexed like the points: window s owns the
 *   slots from d_seg_off[2s] on):
 *     d_kept_labels[slot of point] = cluster id after erasing clusters with fewer than cluster_min
 *        (clusterMinSample) members and renumbering (:89-117), or -1  (= pClusters_/nClusters_)
 *     d_rep[d_seg_off[2s+pol] + k]  = pid of the representative of kept cluster k: the member of
 *        rank size/2 ordered by (Vector2d::norm(), pid)  (:136-147; the reference's nth_element
 *        picks the same pixel unless two members tie in norm at that rank)
 *     candidates j = 0..n-1 in + cluster order (:283-311): d_cand_pair[2*(d_seg_off[2s]+j)..] =
 *        (+ cluster, - cluster), d_cand_xyr[3*(d_seg_off[2s]+j)..] = centre x, centre y, radius
 *     d_win_info[4s..] = { n candidates, kept + clusters, kept - clusters, status } with status
 *        0 = ok, 1 = extractFeatures would return false before pairing (an empty polarity :62-64
 *        or fewer than need_clusters = rows*cols kept clusters :127-129), 4 = more than 2048 DBSCAN
 *        clusters in one polarity (not handled; no candidates).  The exact extraction (ecal_extract_batch_exact_dev / _ordered_dev
 *        and every composite entry point under ECAL_TIES_REFERENCE) ORs ECAL_WIN_TIE_FALLBACK into the word when some tied
 *        median of the window was decided by the smaller-pid rule because the reference's pick could not be worked out (see
 *        ecal_cluster_order_dev's status 1: a segment beyond its workspace): everything else about the window
 *        is as for status 0, the representative of that cluster may differ from the reference's.  ECAL_WIN_STATUS(w) strips it.
 *   The ordering of the candidates into the pattern grid (cv::findCirclesGrid, :332-353) is not
 *   part of this entry point.
 */
#define ECAL_WIN_TIE_FALLBACK 0x100u
#define ECAL_WIN_STATUS(word) ((word) & 0xFFu)
double ecal_circle_radius_threshold(double width, double height, int rows, int cols, int asymmetric,
                                    double square_size, double circle_radius);
int ecal_extract_batch_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                           const int32_t *d_labels, const uint32_t *d_n_clusters, uint32_t S /*windows*/,
                           uint32_t n_points, uint32_t cluster_min, uint32_t need_clusters, double radius_threshold,
                           int fit_circle, uint32_t knn_num, uint32_t *d_win_info /*[S][4]*/, uint32_t *d_cand_pair /*[n_points][2]*/,
                           double *d_cand_xyr /*[n_points][3]*/, int32_t *d_kept_labels /*[n_points]*/,
                           uint32_t *d_rep /*[n_points]*/, void *stream);

/* ---- the whole per-window body in one call ---------------------------------------------------
 * ecal_detect_fused_dev = ecal_slice_events_dev + ecal_dbscan_batch_dev (over the 2S segments) + ecal_extract_batch_dev
 * with the same arguments, the same output arrays and the same results bit for bit — the body of the reference's worker
 * loop per window (event_camera_calib/test/eventCameraCalib.cpp:49-56: EventFrame constructor, extractFeatures with its two
 * DBSCAN::Run calls).  In the shipped configuration (reference point order, eps < 16, fitCircle == 0) ONE kernel carries a
 * window through all three stages on one compute unit; what that kernel cannot take goes through the stages' later passes
 * as before.  Any other configuration runs the three stage functions one after the other. */
int ecal_detect_fused_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const uint32_t *d_win_lo,
                          const uint32_t *d_win_hi, const uint32_t *d_win_base, uint32_t S, uint32_t max_win_events,
                          uint32_t max_seg_points, uint32_t cap_points, double eps, uint32_t minpts, uint32_t cluster_min,
                          uint32_t need_clusters, double radius_threshold, int fit_circle, uint32_t knn_num,
                          double *d_xy, uint32_t *d_seg_off /*[2S]*/, uint32_t *d_seg_cnt /*[2S]*/, int32_t *d_event_point,
                          int *d_overflow, int32_t *d_labels, uint32_t *d_n_clusters /*[2S]*/, uint32_t *d_win_info /*[S][4]*/,
                          uint32_t *d_cand_pair, double *d_cand_xyr, int32_t *d_kept_labels, uint32_t *d_rep, void *stream);

/* ecal_extract_batch_ordered_dev = ecal_extract_batch_dev with the reference's own choice where a cluster's median rank has an
 * equal-norm rival: d_cluster_order = ecal_cluster_order_dev's output for the same segments (the members' positions inside
 * Clusters[c]); the representative of such a cluster is what libstdc++'s std::nth_element leaves at Clusters[c][size / 2]
 * (CirclesEventFrame.cpp:136-147; introselect restated), everything downstream follows.  Clusters of segments
 * ecal_cluster_order_dev did not take (status 1) keep ecal_extract_batch_dev's rule (the smaller pid) and their window's status
 * word carries ECAL_WIN_TIE_FALLBACK. */
int ecal_extract_batch_ordered_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                                   const int32_t *d_labels, const uint32_t *d_n_clusters, const int32_t *d_cluster_order,
                                   uint32_t S /*windows*/, uint32_t n_points, uint32_t cluster_min, uint32_t need_clusters,
                                   double radius_threshold, int fit_circle, uint32_t knn_num, uint32_t *d_win_info,
                                   uint32_t *d_cand_pair, double *d_cand_xyr, int32_t *d_kept_labels, uint32_t *d_rep,
                                   void *stream);

/* What the composite entry points (ecal_detect_batch, ecal_detect_pass, ecal_detect_keyframes, ecal_detect_stream_tiled) do where
 * a kept cluster's median rank has an equal-norm rival: ECAL_TIES_REFERENCE (default) = the reference's own pick
 * (ecal_extract_batch_exact_dev), ECAL_TIES_SMALLER_PID = the cheaper rule of ecal_extract_batch_dev. */
#define ECAL_TIES_REFERENCE 0
#define ECAL_TIES_SMALLER_PID 1
int ecal_set_median_ties(ecal_ctx *ctx, int mode);
int ecal_get_median_ties(const ecal_ctx *ctx);

/* How the stage calls (slicing, DBSCAN, extraction, member order) schedule their later size tiers.  Every stage runs a first-pass
 * kernel that takes what the shipped configuration produces and lists the rest for tiers of growing capacity; on most data
 * those lists stay empty, and a launch that finds its list empty still costs ~5 us (twenty of them: 0.1 ms of every pass).
 * ECAL_TAIL_AUTO (default): a stage whose previous call on this context saw empty lists launches ONE kernel that takes
 * whatever is listed through its most general tier; slicing and DBSCAN, when the first pass listed work but the later hash /
 * pixel passes left none, run those passes + that one kernel; a stage that saw work behind the second pass launches every tier.
 * ECAL_TAIL_TIERED / ECAL_TAIL_LEAN force one form (tests).  The adaptive search (ecal_detect_keyframes), whose windows are
 * second-tier work by design, keeps AUTO but never takes the one-kernel form.
 * The choice moves time only: every listed window is processed either way, results are bit-identical
 * (tests/test_gpu_tail_modes.py). */
/* roctx ranges around the stage entry points (window bounds, slicing, DBSCAN, extraction, member order, grid ordering, keyframe
 * search, init calibration, solver evaluations and solves): on != 0 looks the marker library up at run time
 * (librocprofiler-sdk-roctx.so, else libroctx64.so; ECAL_ERR_INVALID when neither is there), `rocprofv3 --marker-trace
 * --kernel-trace` then attributes every kernel to its stage call.  ECAL_ROCTX=1 in the environment at ecal_init does the same. */
int ecal_set_profile_ranges(ecal_ctx *ctx, int on);

#define ECAL_TAIL_AUTO 0
#define ECAL_TAIL_TIERED 1
#define ECAL_TAIL_LEAN 2
int ecal_set_tail_mode(ecal_ctx *ctx, int mode);
/* the mode in force (ECAL_TAIL_*), or ECAL_ERR_INVALID: lets a caller that switches modes for one stage put back what it found */
int ecal_get_tail_mode(const ecal_ctx *ctx);

/* ecal_extract_batch_exact_dev: the exact extraction in one call (eps = the DBSCAN radius the labels were made with): the plain
 * pass lists the windows in which some kept cluster's median is tied in norm (a third of them on recorded-like data, all of
 * them on the dense benchmark stream),
 * ecal_cluster_order_list_dev works out the reference's member order for the tied clusters of those windows only, and the
 * listed windows are extracted again with it.  Results = ecal_extract_batch_ordered_dev's = the reference's own. */
int ecal_extract_batch_exact_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                                 const int32_t *d_labels, const uint32_t *d_n_clusters, uint32_t S /*windows*/, uint32_t n_points,
                                 double eps, uint32_t cluster_min, uint32_t need_clusters, double radius_threshold, int fit_circle,
                                 uint32_t knn_num, uint32_t *d_win_info, uint32_t *d_cand_pair, double *d_cand_xyr,
                                 int32_t *d_kept_labels, uint32_t *d_rep, void *stream);
/* ecal_cluster_order_dev restricted to the segments 2 w, 2 w + 1 of the windows w = d_win_list[0 .. *d_win_count) (device memory;
 * an entry with bit 30 / bit 31 set: without segment 2 w / 2 w + 1, whose d_order and d_status entries are then left as they are) */
int ecal_cluster_order_list_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, uint32_t S,
                                double eps, const int32_t *d_labels, const uint32_t *d_n_clusters, int32_t *d_order,
                                uint32_t *d_status, int only_tied_medians, const uint32_t *d_win_list, const uint32_t *d_win_count,
                                void *stream);

/* ---- host-buffer conveniences (what the C++ shims in eventcalib_amd/csrc/host/ call) ----------
 * ecal_stream: the event stream uploaded once and kept in HBM — the counterpart of the reference's
 *   EventContainer (event/include/opengv2/event/EventContainer.hpp:25-30), filled once by the driver
 *   (event_camera_calib/test/eventCameraCalib.cpp:154-163) and shared read-only by all workers.
 *   `events` = packed 25-byte records, any order: like the reference's multimap (eventCameraCalib.cpp:154-163) the
 *   stream is brought into time order (stable for equal time stamps; one device sort, only when it is not sorted already).
 * ecal_detect_batch: for every window [t0[s], t1[s]] the EventFrame constructor followed by
 *   extractFeatures up to the candidate circles (the four device entry points above, in order) and
 *   copies the requested results to host memory.  Every pointer of ecal_detect_result may be NULL
 *   (not copied); the layouts are those documented at the device entry points; cap_points must be
 *   >= the total number of events covered by the windows (ECAL_ERR_RANGE otherwise).
 */
typedef struct ecal_stream ecal_stream;
typedef struct ecal_detect_params {
    double dbscan_eps;               /* example.yaml: dbscan_eps */
    uint32_t dbscan_min_samples;     /* dbscan_startMinSample */
    uint32_t cluster_min_sample;     /* clusterMinSample */
    uint32_t need_clusters;          /* BoardSize_Rows * BoardSize_Cols */
    double circle_radius_threshold;  /* ecal_circle_radius_threshold(...) */
    int fit_circle;                  /* fitCircle */
    uint32_t knn_num;                /* knn_num (used when fit_circle != 0) */
    uint32_t rows, cols;             /* BoardSize_Rows / BoardSize_Cols: grid ordering runs when both are > 0 */
} ecal_detect_params;
typedef struct ecal_detect_result {
    uint32_t *win_lo, *win_hi; /* [S] */
    uint32_t *win_base;        /* [S+1] */
    double *xy;                /* [cap_points][2] */
    uint32_t *seg_off, *seg_cnt; /* [2S] */
    int32_t *event_point;      /* [cap_points] */
    int32_t *labels;           /* [cap_points] */
    uint32_t *n_clusters;      /* [2S] */
    int32_t *kept_labels;      /* [cap_points] */
    uint32_t *rep;             /* [cap_points] */
    uint32_t *win_info;        /* [S][4] */
    uint32_t *cand_pair;       /* [cap_points][2] */
    double *cand_xyr;          /* [cap_points][3] */
    int32_t *grid_order;       /* [S][rows*cols] (ecal_grid_order_dev), when params.rows * params.cols > 0 */
    uint32_t *grid_found;      /* [S] */
} ecal_detect_result;
int ecal_stream_create(ecal_ctx *ctx, const uint8_t *events, uint64_t n_events, ecal_stream **out);
/* The same from a .bin file of 25-byte records (EventStream's format): the loop of eventCameraCalib.cpp:154-163 — records with
 * timeStamp >= start_time are kept, and with has_end != 0 the first record with timeStamp >= end_time ends the reading —
 * without a host copy of the file: chunks are read by a few threads into pinned buffers while the previous chunk uploads. */
int ecal_stream_create_from_file(ecal_ctx *ctx, const char *path, double start_time, int has_end, double end_time, ecal_stream **out);
/* time stamps of the first and the last record (both 0 for an empty stream) */
int ecal_stream_times(const ecal_stream *s, double *first, double *last);
void ecal_stream_destroy(ecal_stream *s);
uint64_t ecal_stream_size(const ecal_stream *s);
/* DEVICE pointer of the packed records (what the _dev entry points take as d_events) */
const uint8_t *ecal_stream_data(const ecal_stream *s);
/* the records of the stream as a .bin file (the reference's image: packed 25-byte records), through pinned staging; waits */
int ecal_stream_to_bin_file(ecal_ctx *ctx, const ecal_stream *s, const char *bin_path);
/* device-to-device copy on `stream` (optionally followed by a stream synchronise) */
int ecal_copy_dev(ecal_ctx *ctx, void *d_dst, const void *d_src, size_t bytes, void *stream, int sync);
int ecal_detect_batch(ecal_ctx *ctx, const ecal_stream *es, const double *t0, const double *t1, uint32_t S,
                      const ecal_detect_params *prm, uint32_t cap_points, ecal_detect_result *res);

/* ---- double-buffered ingest (BASELINE configs[4]: hipMemcpyAsync double-buffered ingest) -----------------
 * ecal_detect_stream_tiled: detection over a HOST-resident event file without uploading it first.  Tiled windows
 *   s = [t_start + s len, nextafter(t_start + (s + 1) len, -inf)] (policy P1 of SURVEY 8d: every event in exactly one
 *   window; the reference's piece loop `eventCameraCalib.cpp:172-190` with non-overlapping frames).  Chunks of
 *   windows_per_chunk windows are uploaded with hipMemcpyAsync on a copy stream into one of two device buffers while
 *   the detection kernels (bounds -> slice -> DBSCAN -> candidates -> grid order) of the previous chunk run; pass pinned
 *   host memory (ecal_pin_host, or any hipHostMalloc'ed buffer) — pageable memory makes the copies synchronous.
 *   Outputs (host, any may be NULL): win_info [S][4] as ecal_extract_batch_dev, grid_found [S], features
 *   [S][rows*cols][3] = the ordered circles (centre x, y, radius; NaN where no grid was found).
 *   *n_windows = S = floor((t_last - t_start) / len) + 1 (ECAL_ERR_RANGE if > max_windows). */
typedef struct ecal_ingest_stats {
    uint32_t chunks;
    uint64_t max_chunk_events, bytes_uploaded;
    double seconds;   /* wall time of the whole call */
} ecal_ingest_stats;
/* d_feat [S][M][3] = the ordered circles of every window (candidate d_order[s][k] of window s: centre x, y, radius),
 * NaN where status != 0 or no grid was found; inputs as written by ecal_extract_batch_dev / ecal_grid_order_dev */
int ecal_gather_features_dev(ecal_ctx *ctx, const uint32_t *d_win_info, const uint32_t *d_seg_off, const double *d_cand_xyr,
                             const int32_t *d_order /*[S][M]*/, const uint32_t *d_found, uint32_t S, uint32_t M /*rows*cols*/,
                             double *d_feat, void *stream);
/* ecal_detect_pass: one lock-step pass of the adaptive-window driver (MultiProcess::process, event_camera_calib/test/
 * eventCameraCalib.cpp:49-95, for every active piece at once): the five detection stages + grid ordering over S windows of a
 * DEVICE-resident stream, one upload of the window bounds and ONE download of what the driver's control flow needs:
 * packed [S][3 + 3 rows*cols] doubles = { status (win_info[3]), 1 if extractFeatures() would return true, unique pixels
 * (EventFrame::eventsNum()), then the ordered circles x y r (NaN if none) }.  Synchronous. */
int ecal_detect_pass(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const double *t0, const double *t1, uint32_t S,
                     const ecal_detect_params *prm, uint32_t cap_points, double *packed);
/* ecal_detect_keyframes: the whole adaptive-window driver with the policy on the device — the reference's worker loop
 * (MultiProcess::process, event_camera_calib/test/eventCameraCalib.cpp:34-97: success / slide / grow rule :49-95) over
 * piece_num pieces of [start_time, end_time] (:168-179) with the keyframe gate of EventCalibIni::track (event_camera_calib/
 * src/EventCalibIni.cpp:23-97) against the previous keyframe of the window's own piece or, in the reference's single-worker
 * semantics, of the one shared map (ecal_adaptive_params.gate_mode).  Every lock-step pass = bounds, slicing, DBSCAN, candidates, grid ordering over a CHAIN of
 * windows per piece — its current one and the windows that follow it if every verdict is the likely one: no keyframe, grow
 * (or slide once the window is longer than three lengths); the window slots of a pass, a few per piece in all, go to the
 * pieces still at work — + one policy kernel that applies the rule along that chain for as long as the verdicts are the
 * likely ones (nine in ten are): many windows of a piece's chain per pass, same keyframes as one by one.  All enqueued back to back; the host follows a 4-byte counter check_every passes behind.
 * d_events: DEVICE-resident stream.  cap_points >= the events covered by the windows of any one pass
 * (ecal_detect_keyframes_cap_hint; ECAL_ERR_RANGE otherwise: call again with more).  Outputs (host), sorted by time stamp: kf_time [K], kf_duration
 * [K][2], kf_events_num [K] (EventFrame::eventsNum()), kf_features [K][rows*cols][3] (x, y, radius in grid order);
 * *n_keyframes = K (ECAL_ERR_RANGE with the needed count if K > max_keyframes); *passes = the longest chain of windows
 * a piece went through (the lock-step passes of the one-window-per-pass form; max_passes bounds it), *windows = windows the
 * rule was applied to (the ones evaluated ahead and not taken do not count).  Synchronous; runs on the context's own stream: d_events must be
 * complete when the call is made (no pending writes on other streams). */
typedef struct ecal_adaptive_params {
    double motion_time_step;             /* MotionTimeStep: window = 3 steps, gap after a keyframe = 5 steps */
    uint32_t frame_event_num_threshold;  /* FrameEventNumThreshold */
    uint32_t piece_num;                  /* the reference: 5 * (hardware threads - 2) */
    double start_time, end_time;         /* StartTime / EndTime */
    uint32_t max_passes;                 /* 0 = unlimited */
    uint32_t check_every;                /* passes the host may run ahead of the device's active-piece counter (0 = 2, at most 8) */
    int gate_mode;                       /* ECAL_GATE_OWN_PIECE / ECAL_GATE_SHARED_MAP (below) */
    /* piece_count != 0: only the pieces piece_first .. piece_first + piece_count - 1 of the piece_num pieces (piece 0 is the last
     * in time, eventCameraCalib.cpp:172-179), with exactly the bounds they have in the whole run.  Pieces are independent under
     * ECAL_GATE_OWN_PIECE, so several calls — one context and host thread each — share one search: their kernels overlap on the
     * GPU (a lock-step pass is latency bound) and the union of their keyframes is the whole run's.  With ECAL_GATE_SHARED_MAP a
     * subset needs the frame of the pieces before it: ecal_detect_keyframes_sharded. */
    uint32_t piece_first, piece_count;
} ecal_adaptive_params;
/* Which keyframe a successful window is gated against (EventCalibIni::track, EventCalibIni.cpp:26-36: the map's
 * lower_bound(time stamp), else its last keyframe; TrackingBase.cpp:18-27: only the very first frame is ungated):
 *   ECAL_GATE_OWN_PIECE   the previous keyframe of the window's own piece; every piece's first success is accepted ungated.
 *                         Deterministic and schedule-free, but not what any run of the reference computes.
 *   ECAL_GATE_SHARED_MAP  the reference run with ONE worker thread (threadNum = 1): one map, pieces in pop_back order =
 *                         ascending time, so the reference frame is the map's last keyframe — across piece boundaries too; only
 *                         the first success of the whole run is ungated.  == oracle/policy_oracle.cpp mode 1.  (With several
 *                         workers the reference's result depends on the thread schedule: no deterministic counterpart.) */
#define ECAL_GATE_OWN_PIECE 0
#define ECAL_GATE_SHARED_MAP 1
/* libstdc++'s std::nth_element on doubles with operator< (NaNs compare false), restated — what the gate's median is
 * (EventCalibIni.cpp:78); exported for verification against the real library (host only, no GPU) */
void ecal_ref_nth_element_f64(double *a, uint32_t n, uint32_t nth);
int ecal_detect_keyframes(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_adaptive_params *ap,
                          const ecal_detect_params *prm, uint32_t cap_points, uint32_t max_keyframes, double *kf_time,
                          double *kf_duration, int32_t *kf_events_num, double *kf_features, uint32_t *n_keyframes,
                          uint32_t *passes, uint64_t *windows);
/* ecal_detect_keyframes_sharded: the shared-map search of ONE stream cut over several callers (one per GPU): this call runs the
 * pieces ap->piece_first .. piece_first + piece_count - 1 (contiguous in time) under ECAL_GATE_SHARED_MAP.  What they need from
 * the pieces before them (larger indices = earlier in time, another caller's) is one frame — the map's last keyframe as
 * EventCalibIni::track reads it (EventCalibIni.cpp:26-36): time stamp + the pattern rows' line directions —, so the callers form
 * a chain in time: recv delivers the frame behind all earlier pieces (return 1: *frame filled — has = 0: no keyframe before —,
 * 0: not there yet (only when wait == 0), < 0: error; polled between passes, then waited for; never called by the caller that
 * holds the run's first piece), send is called once with the frame behind this caller's pieces (return < 0: error).  The union
 * of the callers' keyframes == ecal_detect_keyframes over all pieces, record for record.  N - 1 messages of 8 (2 + 2 rows)
 * bytes per search; a caller's pieces run speculatively until its frame arrives (docs: design/11_keyframe_gate.md). */
#define ECAL_FRAME_MAX_ROWS 32
typedef struct ecal_keyframe_frame {
    int has;                              /* 0: no keyframe */
    double time;                          /* KeyFrame time stamp */
    double dir[2 * ECAL_FRAME_MAX_ROWS];  /* [rows][2]: direction of the line fitted to every pattern row (EventCalibIni.cpp:46-57) */
} ecal_keyframe_frame;
typedef int (*ecal_frame_recv_fn)(void *user, ecal_keyframe_frame *frame, int wait);
typedef int (*ecal_frame_send_fn)(void *user, const ecal_keyframe_frame *frame);
typedef struct ecal_adaptive_handover {
    ecal_frame_recv_fn recv;
    ecal_frame_send_fn send;
    void *user;
} ecal_adaptive_handover;
int ecal_detect_keyframes_sharded(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_adaptive_params *ap,
                                  const ecal_detect_params *prm, uint32_t cap_points, uint32_t max_keyframes, double *kf_time,
                                  double *kf_duration, int32_t *kf_events_num, double *kf_features, uint32_t *n_keyframes,
                                  uint32_t *passes, uint64_t *windows, const ecal_adaptive_handover *ho);
/* a cap_points that ecal_detect_keyframes will usually find sufficient for a stream of n_events events (0: invalid
 * parameters); ECAL_ERR_RANGE still says when it was not — double it and call again */
uint64_t ecal_detect_keyframes_cap_hint(const ecal_adaptive_params *ap, uint64_t n_events);
/* ... from the events of the resident stream that lie in [start_time, end_time] (n_events above = events IN that range: a
 * search over part of a stream is sized for that part).  Synchronous on the context's stream; 0 on an error */
uint64_t ecal_detect_keyframes_cap_hint_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_adaptive_params *ap);
int ecal_pin_host(ecal_ctx *ctx, void *ptr, size_t bytes);   /* hipHostRegister */
int ecal_unpin_host(ecal_ctx *ctx, void *ptr);
int ecal_detect_stream_tiled(ecal_ctx *ctx, const uint8_t *events /*host*/, uint64_t n_events, double t_start, double window_len,
                             uint32_t windows_per_chunk, const ecal_detect_params *prm, uint32_t max_windows,
                             uint32_t *win_info, uint32_t *grid_found, double *features, uint32_t *n_windows,
                             ecal_ingest_stats *stats);

/* ---- grid ordering of the candidates -----------------------------------------------------------------
 * Replaces cv::findCirclesGrid(points, Size(cols, rows), centers, CALIB_CB_ASYMMETRIC_GRID[|CLUSTERING]) and the
 * nearest-candidate lookup after it (event_camera_calib/src/CirclesEventFrame.cpp:332-353; the finder is the
 * reference's vendored OpenCV code, cv_calib/src/circlesgrid.cpp) for all windows at once.
 * Inputs: d_win_info / d_seg_off / d_cand_xyr as written by ecal_extract_batch_dev.  Per window s:
 *   d_found[s] = 1 and d_order[s*rows*cols + i*cols + j] = index (into the window's candidate list) of the
 *   circle at model point ((2j + i%2) s, i s, 0) (EventCalibIni.cpp:102-106) — the reference's orderIdxs —
 *   or d_found[s] = 0 and -1 entries when no complete grid is found (extractFeatures returns false).
 * Deterministic lattice walk, not OpenCV's randomised (kmeans) search: same ordering whenever a complete
 * grid is present and seen from its front; parity with the third-party finder is otherwise unpinned.
 * Candidates: up to 128 per window; a window with fewer than rows*cols or more than 128 gets d_found = 0.
 * Pattern shapes: rows >= 2, cols >= 2, rows*cols <= 128 and cols - 1 + rows / 2 <= 28 (integer division).  The last bound is
 *   the walk's: it places the circles on a window of 32 x 32 lattice cells around its seed, the candidate nearest the centroid;
 *   the board spans cols - 1 + rows / 2 cells along its longer lattice diagonal, and must fit with the seed up to one cell off
 *   the middle (so 4 x 27, 3 x 28, 5 x 25, 16 x 8 and 50 x 2 are handled; 4 x 28, 4 x 32 and 2 x 64 are not).  Any other shape
 *   is ECAL_ERR_INVALID, ecal_last_error names the shape and the limit — here, in ecal_grid_order, ecal_detect_pass,
 *   ecal_detect_keyframes[_sharded] and ecal_detect_stream_tiled alike (one check, on the host, before any work is done; the
 *   grid stage of ecal_detect_batch makes it too).
 *   A view whose perspective or off-board clutter moves the centroid more than a cell off the board's middle can still lose a
 *   board of span 27 or 28 (d_found = 0); boards of span <= 26 (5 x 25) have a second cell to spare.
 * Self-symmetric boards: a pattern with an EVEN number of rows maps onto itself under a half turn, (i, j) -> (rows - 1 - i,
 *   cols - 1 - j), so a complete grid has two valid assignments (with odd rows, 9 x 4 among them, exactly one).  The one returned:
 *   that in which the step from the walk's seed to the seed's nearest neighbour goes one column step to the RIGHT on the board
 *   (from model x to x + 1, one row up or down).  It follows from the candidates alone — not from the image's orientation, which
 *   the noise on the seed's four diagonal neighbours outweighs —, and is the same in both launch forms and on every call.
 *   (Mechanism: that step is the walk's first axis, and the pattern is matched through the table of lattice transforms in order;
 *   the first two entries map that axis to the model's (+1, +1) and (+1, -1) diagonals, and one of them always fits such a board.)
 * Hole tolerance: a candidate takes a hole when it lies within min(20 px, 0.7 x the lattice's local step) of the predicted
 *   position, the step being the shorter of the two lattice vectors the walk holds there. */
int ecal_grid_order_dev(ecal_ctx *ctx, const uint32_t *d_win_info, const uint32_t *d_seg_off, const double *d_cand_xyr,
                        uint32_t S, uint32_t rows, uint32_t cols, int32_t *d_order /*[S][rows*cols]*/,
                        uint32_t *d_found /*[S]*/, void *stream);
/* Host-buffer form for one candidate list — the call cv::findCirclesGrid(points, Size(cols, rows), centers,
 * CALIB_CB_ASYMMETRIC_GRID [| CALIB_CB_CLUSTERING]) of CirclesEventFrame.cpp:332-336 (cv_calib/include/cv_calib.hpp:19-21):
 * cand_xyr [n][3] (x, y, radius; the radius is not used), order [rows * cols] = candidate index of every pattern point
 * (-1 when *found == 0).  eventcalib_amd/csrc/host/cv_calib.hpp wraps it in that very signature.  Synchronous. */
int ecal_grid_order(ecal_ctx *ctx, const double *cand_xyr, uint32_t n, uint32_t rows, uint32_t cols, int32_t *order, uint32_t *found);

/* ---- re-detection of the circles around their predicted projections ---------------------------------
 * Replaces CirclesEventFrame::rectifyFeatures(outlierIdxs, Rcw, tcw) (event_camera_calib/src/
 * CirclesEventFrame.cpp:417-638; caller EventCalibIni.cpp:294) for F keyframes at once.  Keyframe f is window
 * d_frame_window[f] of the slicing / DBSCAN / extraction outputs (d_xy, d_seg_off, d_seg_cnt, d_kept_labels =
 * pClusters_/nClusters_ membership, d_win_info); d_pose[12f..] = Rcw row-major (9) then tcw (3), the pose
 * solvePnPRansac gave it (EventCalibIni.cpp:258-272); d_landmarks [rows*cols][3] = landmark positions in grid
 * order (EventCalibIni.cpp:102-106; narrowed to float as the reference's cv::Point3f).  Per circle k:
 *   d_feat_valid[f*n + k] = 0 if the reference erases the feature (projection outside the image :457-461, fewer
 *   than 5 events of either polarity :560-563, refit too far from the prediction :572-576), else 1 and
 *   d_feat_xyr[3(f*n + k)..] = rectified centre x, y, radius (NaN when erased).
 *   d_frame_info[2f..] = { return value of rectifyFeatures (border score :587-622 with fit_circle == 0, 20 % rule
 *   :625-627), number of erased features }.
 * A keyframe whose window has status 4, or more than 2048 kept clusters in a polarity (d_win_info words 1 and 2), is not
 * worked on and comes back all erased: d_feat_valid 0 and d_feat_xyr NaN for every circle, d_frame_info = { 0, rows*cols };
 * ECAL_WIN_TIE_FALLBACK in the status word changes nothing (the window counts as status 0).
 * The outlierIdxs argument of the reference is unused there and has no counterpart.  d_feat_xyr of the accepted
 * keyframes is what ecal_associate_dev takes as d_kf_circles (NaN rows never match an event).
 * cv::projectPoints (OpenCV, third party) is restated: 5 distortion coefficients k1 k2 p1 p2 k3. */
typedef struct ecal_rectify_params {
    double fx, fy, cx, cy;     /* camera->K() */
    double dist[5];            /* camera->distCoeffs(): k1 k2 p1 p2 k3 */
    double width, height;      /* camera->size() */
    uint32_t rows, cols;       /* BoardSize_Rows / BoardSize_Cols, rows*cols <= 128 */
    int asymmetric;            /* pattern_->isAsymmetric */
    double circle_radius;      /* Circles_Radius (world units) */
    int fit_circle;            /* params_.fitCircle: != 0 skips the border-score test */
    int model;                 /* 0: cv::projectPoints with dist = k1 k2 p1 p2 k3 (the reference); 1: cv::fisheye::projectPoints
                                  with dist[0..3] = k1..k4 (BASELINE configs[4]; the reference hands its fisheye coefficients to
                                  the pinhole projection, EventCalibIni.cpp:258 / CirclesEventFrame.cpp:449 — not reproduced) */
} ecal_rectify_params;
int ecal_rectify_batch_dev(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt,
                           const int32_t *d_kept_labels, const uint32_t *d_win_info, const uint32_t *d_frame_window /*[F]*/,
                           const double *d_pose /*[F][12]*/, uint32_t F, const double *d_landmarks /*[rows*cols][3]*/,
                           const ecal_rectify_params *prm, double *d_feat_xyr /*[F][rows*cols][3]*/,
                           uint32_t *d_feat_valid /*[F][rows*cols]*/, uint32_t *d_frame_info /*[F][2]*/, void *stream);
/* host-buffer form: keyframe f owns segments 2f (positiveEvents_) and 2f+1 (negativeEvents_) of xy / kept_labels */
int ecal_rectify_batch(ecal_ctx *ctx, const double *xy /*[n_points][2]*/, const uint32_t *seg_off /*[2F]*/,
                       const uint32_t *seg_cnt /*[2F]*/, const int32_t *kept_labels /*[n_points]*/, uint32_t n_points,
                       const double *pose /*[F][12]*/, uint32_t F, const double *landmarks, const ecal_rectify_params *prm,
                       double *feat_xyr, uint32_t *feat_valid, uint32_t *frame_info);

/* rectifyFeatures for F keyframes named by their time windows over a resident ecal_stream (durations [F][2]; what the batched
 * path of host/event_calib_ini.hpp calls after solvePnPRansac, EventCalibIni.cpp:281-302): the EventFrame constructor and
 * extractFeatures up to the kept clusters run for every window on the device, then ecal_rectify_batch_dev — only the poses go
 * up and the rectified circles (feat_xyr [F][rows*cols][3], feat_valid, frame_info [F][2], layouts as above) come back. */
int ecal_rectify_keyframes(ecal_ctx *ctx, const ecal_stream *es, const double *durations /*[F][2]*/, uint32_t F,
                           const ecal_detect_params *detect_prm, const double *poses /*[F][12]*/, const double *landmarks,
                           const ecal_rectify_params *prm, double *feat_xyr, uint32_t *feat_valid, uint32_t *frame_info);

/* ---- event -> residual association ----------------------------------------------------------------
 * Replaces the association loop of EventCalibSpline::optimize (event_camera_calib/src/EventCalibSpline.cpp:
 * 140-192) and CirclesEventFrame::findCenter (include/opengv2/event_camera_calib/CirclesEventFrame.hpp:50-65):
 * every event with t_min <= t <= t_max (the spline's range) looks up the keyframe nearest in time
 * (d_kf_time ascending, accepted if |dt| < max_dt = 5 * MotionTimeStep) and that keyframe's nearest circle
 * centre (d_kf_circles [K][n_circles][3] = cx, cy, radius in pixels, grid order), accepted if
 * | |pixel - centre| - radius | < edge_tol (5 px).  Accepted events are written in event order:
 * d_obs[j] = pixel, d_time[j] = t, d_lm_id[j] = circle index (= landmark index); *d_count = how many
 * (outputs need room for n_events entries).  These arrays are ecal_spline_problem's obs/time/lm_id.
 * Ties (an event equally far from two keyframes, a pixel equally far from two centres) go to the smaller index.
 * d_kf_time is REQUIRED STRICTLY ascending (kf_time[k - 1] < kf_time[k], no NaN): the search compares the first keyframe not
 * before the event with its predecessor only, so repeated times would break the tie rule ([1, 1, 5], t = 2 gives 1, not 0).
 * The _dev forms cannot report a violation from a device table; ecal_associate and ecal_solver_create_from_stream, which take
 * the table from the host, check and return ECAL_ERR_INVALID (ecal_last_error names the keyframe). */
int ecal_associate_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const double *d_kf_time,
                       const double *d_kf_circles, uint32_t n_keyframes, uint32_t n_circles, double t_min, double t_max,
                       double max_dt, double edge_tol, double *d_obs, double *d_time, uint32_t *d_lm_id,
                       uint32_t *d_count, void *stream);

/* The same for ALL spline segments of a calibration in one pass over the stream: d_ranges [R][2] = (t_min, t_max) of segment r
 * (REQUIRED ascending and disjoint — t_min[r] <= t_max[r] < t_min[r + 1]; EventCalibSpline.cpp:318-345 cuts the keyframes at
 * gaps, so the reference's are —: the device finds an event's range by bisection and cannot report a violation from a device
 * table; ecal_solver_create_from_stream, which takes the ranges from the host, checks and returns ECAL_ERR_INVALID);
 * an event inside range r that passes the two
 * gates becomes a residual of segment r: d_seg_id[j] = r.  Outputs in event order = sorted by (segment, time), which is what
 * ecal_solver_create[_dev] takes; *d_count stays on the device (ecal_solver_create_dev reads it there). */
int ecal_associate_ranges_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const double *d_kf_time,
                              const double *d_kf_circles, uint32_t n_keyframes, uint32_t n_circles, const double *d_ranges,
                              uint32_t n_ranges, double max_dt, double edge_tol, double *d_obs, double *d_time, uint32_t *d_lm_id,
                              uint32_t *d_seg_id, uint32_t *d_count, void *stream);

/* host-buffer form: events from an ecal_stream (resident in HBM), keyframe tables and results in host memory;
 * obs/time/lm_id need room for `capacity` records, *count = records found (ECAL_ERR_RANGE if more than capacity: nothing is
 * copied then).  kf_time not strictly ascending (or NaN): ECAL_ERR_INVALID, ecal_last_error names the keyframe. */
int ecal_associate(ecal_ctx *ctx, const ecal_stream *es, const double *kf_time, const double *kf_circles, uint32_t n_keyframes,
                   uint32_t n_circles, double t_min, double t_max, double max_dt, double edge_tol, uint64_t capacity, double *obs,
                   double *time, uint32_t *lm_id, uint64_t *count);

/* ---- continuous-time calibration solve ---------------------------------------------------------
 * Replaces the Ceres problem of EventCalibSpline::optimize (event_camera_calib/src/EventCalibSpline.cpp:
 * 196-247) for both rotation-spline variants (ecal_spline_problem.use_so3): one residual per associated event,
 *   r = | Xw(event pixel; intrinsics, pose(t)) - landmark | - circle_radius
 * (CalibReprojectionError::operator(), EventCalibSpline.hpp:158-229; unDistort :36-63), HuberLoss(huber_a)
 * with huber_a = 0.2 * circle_radius (:205), EigenQuaternionParameterization on the rotation control
 * points (:116-135), Levenberg-Marquardt with the options of :238-243.
 *
 * Parameter vector (doubles): [ fx fy cx cy k1..k5 | q_c (x y z w) for c < n_cp | t_c (x y z) for c < n_cp ],
 * n_cp = seg_cp_off[n_segments] control points; segment g owns control points
 * [seg_cp_off[g], seg_cp_off[g+1]) and the clamped knot vector knots[seg_cp_off[g] + 4g ..] of
 * n_cp_g + 4 entries (degree 3: BsplineReal<4>/<3> of one segment share it, EventCalibSpline.cpp:68-91).
 * Residual records (the output of the association step, EventCalibSpline.cpp:158-192) must be sorted
 * by (segment, time); 32 bytes each on the device (obs 16 + time 8 + landmark 4 + segment 4): spans and
 * basis values are recomputed from the time (BsplineReal.hpp:107-145,208-231).
 *
 * Normal-equation buffer of ecal_solver_evaluate[_dev] (ecal_solver_normal_size doubles, tangent space,
 * Huber-corrected, SUMS over this process's residuals — ranks add theirs with an all-reduce):
 *   [0] cost = sum rho/2 | [1..9] (J^T r)_intr | [10..90] (J^T J)_intr,intr (9x9 row-major, upper part)
 *   then per control point c, 204 doubles: (J^T r)_c [6: d_rot 3, d_trans 3] | (J^T J)_c,intr [6][9] |
 *   (J^T J)_c,c+d [4][6][6] for d = 0..3 (d = 0: upper part).  with_jacobian = 0 fills only [0].
 */
typedef struct ecal_solver ecal_solver;
typedef struct ecal_spline_problem {
    uint32_t n_segments;
    const uint32_t *seg_cp_off; /* [n_segments + 1] */
    const double *knots;        /* [n_cp + 4 n_segments] */
    uint64_t n_res;
    const double *obs;          /* [n_res][2] event pixel */
    const double *time;         /* [n_res] */
    const uint32_t *lm_id;      /* [n_res] index into landmarks */
    const uint32_t *seg_id;     /* [n_res] or NULL (= all segment 0) */
    uint32_t n_landmarks;
    const double *landmarks;    /* [n_landmarks][3] */
    double circle_radius;       /* Circles_Radius */
    double huber_a;             /* 0.2 * circle_radius in the reference */
    int use_so3;                /* useSO3 (eventCameraCalib.cpp:204-208): 0 = quaternion spline + EigenQuaternion-
                                   Parameterization; 1 = cumulative SO3 spline (CalibReprojectionError_SO3,
                                   EventCalibSpline.hpp:65-135) + LocalParameterizationSO3 (q <- q * exp(delta)) */
    int camera_model;           /* ECAL_CAMERA_RADIAL (the reference's unDistort, EventCalibSpline.hpp:36-63: k1..k5 = the
                                   inverse radial polynomial) or ECAL_CAMERA_FISHEYE (BASELINE configs[4], new: the reference's
                                   solver refuses anything else, EventCalibSpline.cpp:97-99): Kannala-Brandt in the same inverse
                                   form — theta = theta_d (1 + k1 theta_d^2 + .. + k5 theta_d^10) with theta_d = |((u-cx)/fx,
                                   (v-cy)/fy)|, ray = (x, y) tan(theta) / theta_d; k1..k5 are initialised from cv::fisheye's
                                   forward k1..k4 by the same series reversion (ecal_inverse_radial_distortion) */
} ecal_spline_problem;
#define ECAL_CAMERA_RADIAL 0
#define ECAL_CAMERA_FISHEYE 1
/* ---- multi-GPU: one process per GPU, one RCCL communicator per context ---------------------------------------
 * The reference has no distributed backend; north_star shards calibration views and spline residuals one batch per GPU
 * and sums the per-view / per-rank normal-equation blocks with an RCCL all-reduce over xGMI.  Rank 0 calls
 * ecal_comm_unique_id and hands the ECAL_COMM_ID_BYTES bytes to the other ranks by any means (a file, a socket, MPI,
 * torch.distributed); then EVERY rank calls ecal_comm_init on its own context (collective: returns when all world_size
 * ranks have joined; one rank per GPU — RCCL refuses two ranks on one device).  Joining changes nothing by itself: a call
 * whose options carry allreduce == NULL stays rank-local.  A collective solve / calibration is asked for explicitly with
 * options.allreduce = ecal_comm_allreduce and options.allreduce_user = the context (ecal_lm_options.rank / world_size =
 * ecal_comm_rank / ecal_comm_size of that context; anything else is ECAL_ERR_INVALID).  ecal_comm_allreduce_sum_dev: d_buf[0 ..
 * n) summed over the ranks in place, enqueued on `stream` (no host synchronisation); a no-op without a communicator. */
#define ECAL_COMM_ID_BYTES 128
int ecal_comm_unique_id(void *id_out /*[ECAL_COMM_ID_BYTES]*/);
int ecal_comm_init(ecal_ctx *ctx, const void *unique_id, int rank, int world_size);
int ecal_comm_destroy(ecal_ctx *ctx);
int ecal_comm_size(const ecal_ctx *ctx);   /* 1 without a communicator */
int ecal_comm_rank(const ecal_ctx *ctx);
int ecal_comm_allreduce_sum_dev(ecal_ctx *ctx, double *d_buf, size_t n_doubles, void *stream);

/* all-reduce of the solver / calibration: any transport with this signature, or ecal_comm_allreduce (user = the ecal_ctx that
 * joined the communicator; ECAL_ERR_COMM if it never did) */
typedef int (*ecal_allreduce_fn)(void *user, double *d_buf, size_t n_doubles, void *stream);
int ecal_comm_allreduce(void *user /*ecal_ctx* */, double *d_buf, size_t n_doubles, void *stream);
typedef struct ecal_lm_options {
    int max_num_iterations;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double initial_trust_region_radius, max_trust_region_radius, min_relative_decrease;
    double min_lm_diagonal, max_lm_diagonal;
    int jacobi_scaling;
    ecal_allreduce_fn allreduce; /* NULL: this rank alone.  ecal_comm_allreduce (+ allreduce_user = ctx): the context's RCCL communicator */
    void *allreduce_user;
    /* distributed == 1 (needs allreduce): every rank owns its OWN spline segments in its own ecal_solver (its residuals,
     * its control points) and only the 9 intrinsics are shared.  Exchanged per evaluation: the 91-double head (cost,
     * intrinsics gradient and block); per linear solve: the 10 x 10 Schur sums of the rank's banded factorisation + a
     * failure flag + one slot per rank (gradient max-norm); per step: four scalars.  Every rank factorises only its own
     * band and returns its own control points; all ranks return the same intrinsics, cost and summary.
     * distributed == 0 with allreduce set: every rank holds the whole parameter vector and the whole normal-equation
     * buffer is summed (residuals of one segment may then be spread over ranks).
     * distributed == 2 (needs allreduce): TIME SHARDS OF ONE SPLINE — every rank builds its ecal_solver with
     * the whole spline layout (one segment) and the residuals of ITS time range, cut at ecal_solver_time_shard_cuts' times, and
     * passes the same start vector.  The control points fall into world_size interiors separated by 3-control-point
     * separators; exchanged per Jacobian evaluation: the 91-double head + the separators' records (612 doubles per cut); per
     * linear solve: the interiors' 46 x 46 Gram blocks (1082 doubles per rank); per step: four scalars; once at the end: the
     * parameter vector.  Every rank factorises its own interior and all return the same, complete solution. */
    int distributed, rank, world_size;
} ecal_lm_options;
/* cut_time [world_size - 1]: rank r owns the residuals with cut_time[r - 1] <= t < cut_time[r] (distributed == 2) */
int ecal_solver_time_shard_cuts(const double *knots /*[n_cp + 4]*/, uint32_t n_cp, int world_size, double *cut_time);
typedef struct ecal_lm_summary {
    int iterations, successful_steps, unsuccessful_steps, jacobian_evaluations, cost_evaluations;
    int termination; /* 0 = converged (a tolerance fired), 1 = max_num_iterations reached */
    double initial_cost, final_cost, seconds;
    double seconds_evaluate;     /* H2D parameters + kernels + all-reduce + D2H buffer, summed */
    double seconds_linear_solve; /* banded-arrow Cholesky + model change on the host, summed */
} ecal_lm_summary;
int ecal_solver_create(ecal_ctx *ctx, const ecal_spline_problem *problem, ecal_solver **out);
/* The problem built in place (EventCalibSpline.cpp:181-235 adds the residual blocks where the association finds them):
 * problem->obs / time / lm_id / seg_id are DEVICE pointers — the outputs of ecal_associate_ranges_dev, consumed when the call
 * returns —, problem->n_res their capacity and *d_n_res (device; NULL: n_res itself) the number of residuals; the other members
 * (seg_cp_off, knots, landmarks) stay host pointers.  Records and chunk table are made by kernels on `stream`; one 12-byte
 * read-back.  Same solver object, same checks (ECAL_ERR_INVALID) as ecal_solver_create. */
int ecal_solver_create_dev(ecal_ctx *ctx, const ecal_spline_problem *problem, const uint32_t *d_n_res, void *stream,
                           ecal_solver **out);
uint64_t ecal_solver_num_residuals(const ecal_solver *s);
/* Host-pointer convenience of the two (what host/event_calib_spline.hpp calls): the association of every spline segment over a
 * resident ecal_stream + the solver built on the result, the residual arrays never leaving HBM.  kf_time / kf_circles / ranges
 * [n_ranges][2] are host tables (ecal_associate_ranges_dev's arguments); layout = the problem without its residual arrays (obs,
 * time, lm_id, seg_id, n_res ignored); n_ranges must equal layout->n_segments.  ecal_solver_num_residuals says how many were found.
 * ECAL_ERR_INVALID (ecal_last_error names the entry) if the ranges are not ascending and disjoint or kf_time is not strictly ascending. */
int ecal_solver_create_from_stream(ecal_ctx *ctx, const ecal_stream *es, const double *kf_time, const double *kf_circles,
                                   uint32_t n_keyframes, uint32_t n_circles, const double *ranges, uint32_t n_ranges, double max_dt,
                                   double edge_tol, const ecal_spline_problem *layout, ecal_solver **out);
void ecal_solver_destroy(ecal_solver *s);
size_t ecal_solver_param_size(const ecal_solver *s);
size_t ecal_solver_normal_size(const ecal_solver *s);
uint32_t ecal_solver_num_chunks(const ecal_solver *s);
int ecal_solver_evaluate_dev(ecal_solver *s, const double *d_params, int with_jacobian, double *d_accum, void *stream);
int ecal_solver_evaluate(ecal_solver *s, const double *params, int with_jacobian, double *accum);
/* The Ceres CostFunction::Evaluate seam (CalibReprojectionError{,_SO3}::Create, EventCalibSpline.hpp:137-146,231-240:
 * AutoDiffCostFunction<..., 1, 9, 4, 4, 4, 4, 3, 3, 3, 3> + EigenQuaternionParameterization / LocalParameterizationSO3) for
 * every residual of the problem at `params`: r[k] = the raw residual (no loss function); J[k][33] (optional) = the raw row
 * of the tangent-space Jacobian, columns [ intrinsics 9 | rotation tangent of control points cp0[k] .. cp0[k]+3, 3 each |
 * translation of the same four, 3 each ]; cp0[k] (optional) = the first of the four control points residual k touches. */
int ecal_residuals_dev(ecal_solver *s, const double *d_params, double *d_r /*[n_res]*/, double *d_J /*[n_res][33] or NULL*/,
                       uint32_t *d_cp0 /*[n_res] or NULL*/, void *stream);
int ecal_residuals(ecal_solver *s, const double *params, double *r, double *J, uint32_t *cp0);
/* Calibration quality report: the raw residuals of the problem at `params` (the r of ecal_residuals, no loss function) binned on
 * the GPU in one pass over the solver's records — which keyframes fit badly, which circles of the board, which parts of the
 * sensor were never covered — a few kilobytes out instead of one double per residual.  Residuals are in BOARD UNITS, the unit of
 * ecal_spline_problem.circle_radius (a distance on the board plane), not pixels.
 *   totals    all residuals; cost = sum rho(r^2) / 2 with the solver's Huber loss = [0] of ecal_solver_evaluate(with_jacobian = 0)
 *   kf        [n_keyframes]: a residual counts for the keyframe nearest in time in the ascending table kf_time [n_keyframes]
 *             (all segments in one table), by the association's rule: the first index with kf_time >= t against its predecessor,
 *             the predecessor when d0 * d0 <= d1 * d1; no max_dt gate: every residual lands in exactly one keyframe
 *   lm        [n_landmarks], indexed by lm_id (at most 1024 landmarks: ECAL_ERR_RANGE)
 *   cell_n / cell_sum_r2 [cells_y][cells_x], cells_x = ceil(width / cell_px), cells_y = ceil(height / cell_px): the sensor in
 *             square cells, cell_x = min((uint32) max(u, 0) / cell_px, cells_x - 1), the same for y; cell_px == 0 or more than
 *             8192 cells is ECAL_ERR_INVALID
 *   hist      [hist_bins], 1 <= hist_bins <= 256: bin = clamp((int) floor((r + hist_range) * hist_bins / (2 hist_range)), 0,
 *             hist_bins - 1): the first and the last bin catch the tails
 * n_out counts the residuals with |r| > outlier_thresh.  Any output but the totals may be NULL: that family is skipped (and its
 * options are not looked at).  n_keyframes == 0 with a kf output is ECAL_ERR_INVALID; a solver without residuals gives zeros.
 * The call zeroes its outputs itself on `stream`; the _dev form takes device pointers and does not synchronise with the host.
 * FP64 sums are accumulated with atomics: they depend on the order of arrival in the last bits, the counts do not. */
typedef struct ecal_report_options {
    uint32_t width, height, cell_px; /* sensor size and the cell's side, pixels */
    uint32_t hist_bins;
    double hist_range;               /* the histogram covers [-hist_range, hist_range); <= 0: 4 * huber_a */
    double outlier_thresh;           /* <= 0: the solver's huber_a */
} ecal_report_options;
typedef struct ecal_bin_stats {
    uint64_t n, n_out;
    double sum_r, sum_r2, sum_abs, max_abs;
} ecal_bin_stats;
typedef struct ecal_report_totals {
    ecal_bin_stats all;
    double cost;
} ecal_report_totals;
void ecal_report_default_options(ecal_report_options *opt); /* 346 x 260, 16 px cells, 64 bins, range and threshold from huber_a */
int ecal_solver_report_dev(ecal_solver *s, const double *d_params, const double *d_kf_time, uint32_t n_keyframes,
                           const ecal_report_options *opt /*NULL: the defaults*/, ecal_report_totals *d_total, ecal_bin_stats *d_kf,
                           ecal_bin_stats *d_lm, uint64_t *d_cell_n, double *d_cell_sum_r2, uint64_t *d_hist, void *stream);
int ecal_solver_report(ecal_solver *s, const double *params, const double *kf_time, uint32_t n_keyframes,
                       const ecal_report_options *opt, ecal_report_totals *total, ecal_bin_stats *kf, ecal_bin_stats *lm,
                       uint64_t *cell_n, double *cell_sum_r2, uint64_t *hist);
uint32_t ecal_solver_num_landmarks(const ecal_solver *s);
/* ---- report in pixels ---------------------------------------------------------------------------------------------------------
 * The same report with every statistic in PIXELS: per residual record the first-order (Sampson) distance from the event to the
 * projected rim of its circle, r_px = r / |d r / d (u, v)|, signed like r.  It is defined wherever the residual is — it does not go
 * through a forward projection, which exists only inside the solved polynomial's monotone radius — and it does not grow with depth
 * or obliquity as the board-unit residual does.  For a residual record (pixel u, v, time, landmark) at `params`, operation by
 * operation:
 *   r        the raw residual of ecal_residuals
 *   gu, gv   d r / d u, d r / d v = the negatives of columns 2 and 3 (cx, cy) of that record's Jacobian row; in residual_core's terms
 *            (spline_residual.hpp) gu = gx * ifx, gv = gy * ify, with no robust loss
 *   g2       gu * gu + gv * gv
 *   degenerate  iff r or g2 is not finite or g2 > 0 is false: the record is counted in n_degenerate and enters no bin
 *   r_px     r / sqrt(g2) otherwise, the division and the square root correctly rounded; px_per_unit = 1 / sqrt(g2)
 * r, gu and gv are compiled the way the solver compiles its residual (contraction to FMA allowed); everything from g2 on, and
 * everything that decides a bin, without contraction.
 * ecal_solver_report_px[_dev]: arguments, families, NULL-skips-the-family rule, keyframe tie rule, limits and error codes of
 * ecal_solver_report[_dev]; every statistic is of r_px and there is no cost.  Options: ecal_report_options with pixel defaults
 * (ecal_report_px_default_options: 346 x 260, 16 px cells, 64 bins, hist_range = 4.0 px, outlier_thresh = 1.0 px — interface
 * choices, not tolerances); a hist_range or outlier_thresh <= 0 passed in a call means these same two values.
 * totals.sum_px_per_unit = the sum of 1 / sqrt(g2) over the non-degenerate records: its mean says how many pixels one board unit
 * is in this data.  all.n + n_degenerate = the solver's residuals.  The call zeroes its outputs itself on `stream`; the _dev form
 * takes device pointers and does not synchronise with the host; the host form stages through the context's scratch.
 * ecal_residuals_px[_dev], the per-event form: r_px [n_res] (0.0 where the record is degenerate), grad [n_res][2] = (gu, gv)
 * (optional), flag [n_res] (optional): 1 = degenerate, 0 otherwise. */
typedef struct ecal_report_px_totals {
    ecal_bin_stats all;
    uint64_t n_degenerate;
    double sum_px_per_unit;
} ecal_report_px_totals;
void ecal_report_px_default_options(ecal_report_options *opt);
int ecal_solver_report_px_dev(ecal_solver *s, const double *d_params, const double *d_kf_time, uint32_t n_keyframes,
                              const ecal_report_options *opt /*NULL: the pixel defaults*/, ecal_report_px_totals *d_total,
                              ecal_bin_stats *d_kf, ecal_bin_stats *d_lm, uint64_t *d_cell_n, double *d_cell_sum_r2, uint64_t *d_hist,
                              void *stream);
int ecal_solver_report_px(ecal_solver *s, const double *params, const double *kf_time, uint32_t n_keyframes,
                          const ecal_report_options *opt, ecal_report_px_totals *total, ecal_bin_stats *kf, ecal_bin_stats *lm,
                          uint64_t *cell_n, double *cell_sum_r2, uint64_t *hist);
int ecal_residuals_px_dev(ecal_solver *s, const double *d_params, double *d_r_px /*[n_res]*/, double *d_grad /*[n_res][2] or NULL*/,
                          uint8_t *d_flag /*[n_res] or NULL*/, void *stream);
int ecal_residuals_px(ecal_solver *s, const double *params, double *r_px, double *grad, uint8_t *flag);
/* Board-frame event image (the motion-compensated image of the calibration): EVERY event of a stream — not only the ones the
 * association kept — carried through the intrinsics of `params` and the pose of the solver's spline at its own time stamp onto
 * the board plane z = 0 (the first half of the residual: inverse camera model, rotation, ray / plane intersection).  With a good
 * calibration the events collapse into sharp rings of radius circle_radius around the landmarks; with a bad one they smear.
 * One pass over the packed, time-sorted 25-byte records; blocks of ECAL_BOARD_IMAGE_BLOCK events per workgroup.  Per event:
 *   segment    the spline segment g with knots_g[3] <= t <= knots_g[n_cp_g] (both ends inclusive); none: n_outside_time
 *              (the segments' time ranges are ascending and disjoint; a time at which two of them touch belongs to the earlier)
 *   board point (Xw0, Xw1) in board units; a ray that does not meet the plane in front of the camera (depth not finite or
 *              <= 0): n_behind
 *   image      ix = floor((Xw0 - x0) / bin), iy = floor((Xw1 - y0) / bin); inside [0, width) x [0, height): img[p][iy][ix]++ with
 *              p = 1 for a positive event (polarity byte != 0), 0 for a negative one, and n_image[p]++; else n_outside_image
 *   ring profile (ring_bins > 0; at most 128 landmarks: ECAL_ERR_RANGE): the landmark nearest in the plane (squared distance,
 *              ties to the lower index), d = |Xw - lm| - circle_radius; when |d| < ring_range: n_ring++,
 *              ring_hist[lm][floor((d + ring_range) * ring_bins / (2 ring_range))]++ and ring_stats[lm][p] += {1, d, d * d}
 * n_events = n_outside_time + n_behind + n_outside_image + n_image[0] + n_image[1].  Every count is an integer atomic and does
 * not depend on the order of arrival; sum_d / sum_d2 do in their last bits.  bin > 0, width * height <= 2^24, ring_bins <= 256,
 * ring_range > 0 when ring_bins > 0 (ECAL_ERR_INVALID otherwise).  Any of d_img / d_ring_stats / d_ring_hist may be NULL (the
 * totals are the same); the call zeroes its outputs itself on `stream`; n_events == 0 is valid.  d_params: the solver's
 * parameter vector (ecal_solver_param_size doubles). */
#define ECAL_BOARD_IMAGE_BLOCK 4096u  /* events per workgroup */
#define ECAL_BOARD_IMAGE_CP_LDS 16u   /* control points a workgroup stages on chip; a block that needs more (a very fine knot
                                         vector) or meets more than one segment reads them from global memory: same results */
typedef struct ecal_board_image_options {
    double x0, y0, bin;     /* board coordinates of the image's corner, side of a pixel (board units) */
    uint32_t width, height; /* pixels */
    uint32_t ring_bins;     /* 0: no ring profile */
    double ring_range;      /* the ring histogram covers d in (-ring_range, ring_range) */
} ecal_board_image_options;
typedef struct ecal_board_image_totals {
    uint64_t n_events, n_outside_time, n_behind, n_outside_image, n_image[2], n_ring;
} ecal_board_image_totals;
typedef struct ecal_ring_stats {
    uint64_t n;
    double sum_d, sum_d2;
} ecal_ring_stats;
/* the landmarks' bounding box padded by 3 radii, bin = radius / 8, ring_bins = 64, ring_range = radius */
int ecal_board_image_default_options(const ecal_solver *s, ecal_board_image_options *opt);
int ecal_solver_board_image_dev(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events,
                                const ecal_board_image_options *opt /*NULL: the defaults*/, uint32_t *d_img /*[2][height][width]*/,
                                ecal_board_image_totals *d_totals, ecal_ring_stats *d_ring_stats /*[n_landmarks][2]*/,
                                uint64_t *d_ring_hist /*[n_landmarks][ring_bins]*/, void *stream);
/* the per-event form (scatter plots; the seam the tests pin the arithmetic through): d_xw [n_events][2] board points (zeros
 * where the flag is not 0), d_flag [n_events]: 0 ok, 1 outside every segment's time range, 2 behind the camera */
int ecal_solver_board_points_dev(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events,
                                 double *d_xw, uint8_t *d_flag, void *stream);
/* host-buffer forms over a resident ecal_stream: params and outputs in host memory, synchronous */
int ecal_solver_board_image(ecal_solver *s, const double *params, const ecal_stream *es, const ecal_board_image_options *opt,
                            uint32_t *img, ecal_board_image_totals *totals, ecal_ring_stats *ring_stats, uint64_t *ring_hist);
int ecal_solver_board_points(ecal_solver *s, const double *params, const ecal_stream *es, double *xw, uint8_t *flag);
/* Re-association through the solved spline: the association in the BOARD frame, at the current solution.  The keyframe
 * association above keeps an event only near a keyframe's time and near the ring that keyframe's circle had at its instant; this
 * pass makes, per event of the packed, time-sorted stream, exactly the board image's decisions — segment (ranges inclusive, a
 * time two segments share to the earlier, a NaN to none: n_outside_time), board point (depth not finite or <= 0: n_behind),
 * nearest landmark (squared distance in the plane, ties to the lower index; at most 128 landmarks: ECAL_ERR_RANGE),
 * d = |Xw - lm| - circle_radius — and KEEPS the event as a residual of that landmark when |d| < ring_tol (else n_off_ring),
 * wherever it sits relative to a keyframe.  Outputs in event order = (segment, time) order, what ecal_solver_create_dev takes:
 * d_obs[j] / d_time[j] = the event's own bytes, d_lm_id[j], d_seg_id[j]; *d_count = how many (device; room for n_events records
 * each).  ring_tol: board units, <= 0 = the solver's huber_a (the convention of ecal_report_options.outlier_thresh), not finite =
 * ECAL_ERR_INVALID.  n_events = n_outside_time + n_behind + n_off_ring + n_kept and n_kept = *d_count; every count is an integer
 * atomic.  The call zeroes *d_count and the totals itself on `stream` and does not synchronise with the host; n_events == 0 is
 * valid; more than 2^32-1 events is ECAL_ERR_RANGE.  Three launches, no waiting between workgroups: a verdict byte per event and
 * a count per block, the scan of the counts, the ordered copy (scratch from the context: one byte per event + the block tables).
 * Rank-local and single-process: the multi-GPU solves (ecal_lm_options.distributed) do not use it. */
typedef struct ecal_reassociate_totals {
    uint64_t n_events, n_outside_time, n_behind, n_off_ring, n_kept;
} ecal_reassociate_totals;
int ecal_solver_reassociate_dev(ecal_solver *s, const double *d_params, const uint8_t *d_events, uint64_t n_events,
                                double ring_tol, double *d_obs, double *d_time, uint32_t *d_lm_id, uint32_t *d_seg_id,
                                uint32_t *d_count, ecal_reassociate_totals *d_totals /*or NULL*/, void *stream);
/* host-buffer form over a resident ecal_stream, synchronous: obs / time / lm_id / seg_id need room for `capacity` records,
 * *count = records found (ECAL_ERR_RANGE if more than capacity: nothing is copied then, as ecal_associate) */
int ecal_solver_reassociate(ecal_solver *s, const double *params, const ecal_stream *es, double ring_tol, uint64_t capacity,
                            double *obs, double *time, uint32_t *lm_id, uint32_t *seg_id, uint64_t *count,
                            ecal_reassociate_totals *totals /*or NULL*/);
/* ... and a NEW solver built in place on those records (ecal_solver_create_dev), with the layout of s — segments, knots,
 * landmarks, radius, Huber width, rotation variant, camera model — from the host copies s keeps: nothing proportional to the
 * events crosses PCIe (the count and the totals come back).  s is left untouched; both solvers are destroyed independently.
 * Scratch from the context: 33 bytes per event plus the block tables. */
int ecal_solver_create_reassociated(ecal_solver *s, const double *params, const ecal_stream *es, double ring_tol,
                                    ecal_solver **out, ecal_reassociate_totals *totals /*or NULL*/);
void ecal_lm_default_options(ecal_lm_options *opt);
int ecal_solver_solve(ecal_solver *s, double *params /*in: start, out: solution*/, const ecal_lm_options *opt,
                      ecal_lm_summary *summary);
/* PinholeCamera::inverseRadialDistortion (core/sensor/src/PinholeCamera.cpp:69-95): (k1,k2,k3,k4) -> the
 * five inverse-polynomial coefficients that initialise k1..k5 (EventCalibSpline.cpp:101-105). */
void ecal_inverse_radial_distortion(const double *k4, double *b5);

/* ---- init calibration on calibration views ---------------------------------------------------------
 * Replaces the OpenCV calls of EventCalibIni::cvCalibration (event_camera_calib/src/EventCalibIni.cpp:149-347):
 *   cv::calibrateCamera(objectPoints, imagePoints, imageSize, K, dist(8), rvecs, tvecs, flag | CALIB_USE_LU)  :198-199
 *   cv::fisheye::calibrate(objectPoints, imagePoints, imageSize, K, dist(4), rvecs, tvecs, flag)              :188
 *   cv::solvePnPRansac(objectPoints[0], imageP, K, dist, rvec, tvec, false, 50, 4.0, 0.99, inliers, IPPE)     :258-259
 * with the flag word assembled as in parameters.hpp:48-69.  OpenCV is third party (not in the reference tree):
 * the algorithms are restated (oracle/calib_oracle.py lists them), parity with OpenCV itself is unpinned.
 *
 * Intrinsics slots (12 doubles): model 0 = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 (cv::calibrateCamera's K and its
 * 8 distortion coefficients in OpenCV's order), model 1 = fx fy cx cy alpha k1 k2 k3 k4 (cv::fisheye).
 * A view = the n_pts circle centres of one keyframe in grid order (CirclesEventFrame::features()); the board
 * points obj [n_pts][3] are calcBoardCornerPositions (EventCalibIni.cpp:99-115) and must have z == 0.
 * Pose of a view: rvec (cv::Rodrigues vector) and tvec, camera <- board.
 *
 * ecal_calib_view_blocks_dev: the data-parallel piece — per view v the normal-equation blocks of its
 *   2 n_pts reprojection residuals r = projected - measured with the analytic Jacobian J (columns of fixed
 *   intrinsics zeroed; with FIX_ASPECT_RATIO fx is tied to aspect_ratio * fy and its column folded into fy's):
 *   d_blocks[272 v ..] = Hii [12][12] | Hiv [12][6] | Hvv [6][6] | gi = (J^T r)_intr [12] | gv [6] | cost = r^T r | pad.
 *   with_jacobian = 0 writes only cost (slot 270).  Blocks of different views are independent: views shard across
 *   GPUs and only Schur-reduced 12 x 12 records are summed (ecal_calibrate_views below).
 * ecal_pnp_batch_dev: planar pose of F frames at once — undistort, homography, IPPE (both solutions, the one with
 *   the smaller reprojection error), `rounds` consensus rounds with inliers = reprojection error <= reproj_thresh
 *   px (0 = none; a deterministic stand-in for the RANSAC loop), then refine_iters Levenberg-Marquardt iterations
 *   on the pose (0 = none, as solvePnPRansac's final SOLVEPNP_IPPE call; 20 = cvFindExtrinsicCameraParams2).
 *   d_valid [F][n_pts] (or NULL) masks missing circles.  d_pose [F][6] = rvec, tvec; d_inlier [F][n_pts];
 *   d_err [F] = sum of squared reprojection errors over the inliers; d_ok [F] = 0 if no pose was found.
 * ecal_calibrate_views: the whole calibration for this process's views (host pointers).  With options.allreduce
 *   set, every rank passes its own shard of the views (n_views may differ, 0 allowed) and all ranks return the
 *   same intrinsics; rvecs / tvecs / per_view_err are those of the local views.
 */
#define ECAL_CALIB_FIX_ASPECT_RATIO    (1u << 0)  /* cv::CALIB_FIX_ASPECT_RATIO: fx = aspect_ratio * fy */
#define ECAL_CALIB_FIX_PRINCIPAL_POINT (1u << 1)  /* cv::CALIB_FIX_PRINCIPAL_POINT / fisheye::CALIB_FIX_PRINCIPAL_POINT */
#define ECAL_CALIB_ZERO_TANGENT_DIST   (1u << 2)  /* cv::CALIB_ZERO_TANGENT_DIST */
#define ECAL_CALIB_FIX_K1              (1u << 3)
#define ECAL_CALIB_FIX_K2              (1u << 4)
#define ECAL_CALIB_FIX_K3              (1u << 5)
#define ECAL_CALIB_FIX_K4              (1u << 6)
#define ECAL_CALIB_FIX_K5              (1u << 7)
#define ECAL_CALIB_FIX_K6              (1u << 8)
#define ECAL_CALIB_FIX_SKEW            (1u << 9)  /* cv::fisheye::CALIB_FIX_SKEW */
#define ECAL_CALIB_RECOMPUTE_EXTRINSIC (1u << 10) /* cv::fisheye::CALIB_RECOMPUTE_EXTRINSIC */
#define ECAL_CALIB_USE_INTRINSIC_GUESS  (1u << 11) /* cv::CALIB_USE_INTRINSIC_GUESS / cv::fisheye::CALIB_USE_INTRINSIC_GUESS: res->intr
                                                     (all 12 slots) is the START of the iteration instead of the models' own
                                                     initialisation (homographies / max(w, h) / pi) */
#define ECAL_CALIB_BLOCK_DOUBLES 272
typedef struct ecal_calib_options {
    int model;            /* 0 = pinhole (Calibrate_UseFisheyeModel: 0), 1 = fisheye */
    uint32_t flags;       /* ECAL_CALIB_* */
    double aspect_ratio;  /* Calibrate_FixAspectRatio (used with ECAL_CALIB_FIX_ASPECT_RATIO) */
    int max_iter;         /* 0 = OpenCV's default TermCriteria: 30 (calibrateCamera) / 100 (fisheye) */
    double eps;           /* 0 = DBL_EPSILON */
    ecal_allreduce_fn allreduce; /* NULL: this rank alone.  ecal_comm_allreduce (+ allreduce_user = ctx): the context's RCCL communicator */
    void *allreduce_user;
} ecal_calib_options;
typedef struct ecal_calib_result {
    double intr[12];
    double rms;           /* sqrt(sum of squared reprojection errors / number of points), all ranks' views */
    int iterations, jacobian_evaluations, error_evaluations;
    double seconds;
} ecal_calib_result;
void ecal_calib_default_options(ecal_calib_options *opt);
int ecal_calib_view_blocks_dev(ecal_ctx *ctx, const double *d_obj /*[n_pts][3]*/, uint32_t n_pts, const double *d_img /*[V][n_pts][2]*/,
                               uint32_t n_views, int model, uint32_t flags, double aspect_ratio, const double *d_intr /*[12]*/,
                               const double *d_view_params /*[V][6]*/, int with_jacobian, double *d_blocks /*[V][272]*/, void *stream);
int ecal_pnp_batch_dev(ecal_ctx *ctx, const double *d_obj, uint32_t n_pts, const double *d_img /*[F][n_pts][2]*/,
                       const uint32_t *d_valid /*[F][n_pts] or NULL*/, uint32_t n_frames, int model, const double *d_intr /*[12]*/,
                       double reproj_thresh, int rounds, int refine_iters, double *d_pose /*[F][6]*/, uint32_t *d_inlier /*or NULL*/,
                       double *d_err /*or NULL*/, uint32_t *d_ok /*or NULL*/, void *stream);
/* host-buffer form of ecal_pnp_batch_dev */
int ecal_pnp_batch(ecal_ctx *ctx, const double *obj, uint32_t n_pts, const double *img, const uint32_t *valid /*or NULL*/,
                   uint32_t n_frames, int model, const double *intr /*[12]*/, double reproj_thresh, int rounds, int refine_iters,
                   double *pose /*[F][6]*/, uint32_t *inlier /*or NULL*/, double *err /*or NULL*/, uint32_t *ok /*or NULL*/);
/* The sequential keyframe gates of EventCalibIni::cvCalibration (event_camera_calib/src/EventCalibIni.cpp:281-302) on results that
 * are known for all keyframes at once (ecal_pnp_batch, ecal_rectify_keyframes): frame f, in time order, is discarded when its PnP
 * failed or EventCalibIni::checkPose (:327-347: translational speed |twb_f - twb_last| / dt below (0.25 / step) * 2 and angular
 * speed |acos((trace(Rsw_f Rsw_last^T) - 1) / 2)| / dt below (5e-4 pi) * 2 / step) fails against the LAST ACCEPTED frame (the first
 * accepted frame has none to be checked against), then when its rectification failed; otherwise it is accepted.  Host code, no
 * context: the loop carries a dependence from frame to frame.  accepted[0 .. *n_accepted) = the accepted frames' indices. */
int ecal_pose_gates(uint32_t n_frames, const double *Rsw /*[F][9] row-major*/, const double *twb /*[F][3]*/, const double *time /*[F]*/,
                    const uint8_t *pnp_ok /*[F]*/, const uint8_t *rect_ok /*[F]*/, double motion_time_step,
                    uint32_t *accepted /*[F]*/, uint32_t *n_accepted, uint32_t *n_discarded_by_check_pose,
                    uint32_t *n_discarded_by_rectify);
int ecal_calibrate_views(ecal_ctx *ctx, const double *obj /*[n_pts][3]*/, uint32_t n_pts, const double *img /*[V][n_pts][2]*/,
                         uint32_t n_views, double width, double height, const ecal_calib_options *opt, ecal_calib_result *res,
                         double *rvecs /*[V][3] or NULL*/, double *tvecs /*[V][3] or NULL*/, double *per_view_err /*[V] or NULL*/);

/* The fisheye init calibration (cv::fisheye::calibrate at EventCalibIni.cpp:186-190) with ONE start procedure for every
 * caller: the reference's own start first (principal point at the centre, f = max(w, h) / pi, no guess); only when that fails —
 * ECAL_ERR_INVALID or a non-finite result — the radial model is calibrated on the same views with
 * ECAL_CALIB_FISHEYE_PRECALIB_FLAGS and its fx, fy, cx, cy start the fisheye model (ECAL_CALIB_USE_INTRINSIC_GUESS).
 * *start_used: 0 the reference's start, 1 the radial guess was needed, 2 the caller's own guess (opt->flags carries
 * ECAL_CALIB_USE_INTRINSIC_GUESS, res->intr the guess).  opt->model is ignored (fisheye). */
#define ECAL_CALIB_FISHEYE_PRECALIB_FLAGS                                                                                  \
    (ECAL_CALIB_FIX_PRINCIPAL_POINT | ECAL_CALIB_ZERO_TANGENT_DIST | ECAL_CALIB_FIX_ASPECT_RATIO | ECAL_CALIB_FIX_K3 | ECAL_CALIB_FIX_K4 | \
     ECAL_CALIB_FIX_K5 | ECAL_CALIB_FIX_K6)
int ecal_calibrate_fisheye_views(ecal_ctx *ctx, const double *obj, uint32_t n_pts, const double *img, uint32_t n_views, double width,
                                 double height, const ecal_calib_options *opt, ecal_calib_result *res, double *rvecs, double *tvecs,
                                 double *per_view_err, int *start_used);

/* ---- initial spline fit + evaluation (host; no GPU involved) -------------------------------------------
 * ecal_spline_fit: BsplineReal<dim>(3, Q, controlPointsNum, u) (core/spline/include/opengv2/spline/
 *   BsplineReal.hpp:17-100,329-449) as EventCalibSpline builds twbSplines_ / QwbSplines_ from the keyframe poses
 *   (event_camera_calib/src/EventCalibSpline.cpp:61-91), and BsplineSO3's knotSpacing + initialGuess
 *   (core/spline/src/BsplineSO3.cpp:60-72,198-279; its Ceres refinement optimizeCP: ecal_spline_so3_refine below).  u [m] ascending sample parameters (timestamps, first and
 *   last already widened by 3 steps as :63-66), data [m][dim]; outputs the clamped knot vector [n_cp + 4]
 *   (NURBS book 9.68) — the layout ecal_spline_problem.knots takes — and the control points [n_cp][dim]: first and
 *   last interpolate, the interior ones minimise the squared distance at the interior samples.
 *   ECAL_ERR_INVALID if n_cp < 4, m < 2 or a control point has no supporting sample.
 * ecal_spline_eval: BsplineReal::evaluate(u, 0, ..) (:454-470) at m parameters (updateMap, EventCalibSpline.cpp:
 *   253-317); ECAL_ERR_RANGE outside the knot range. */
/* ecal_spline_so3_refine: BsplineSO3::optimizeCP (core/spline/src/BsplineSO3.cpp:285-341) — the control points of the
 *   cumulative cubic SO3 spline (unit quaternions x y z w, [n_cp][4], in: the initial guess of ecal_spline_fit on the
 *   quaternion coefficients, out: refined) fitted on the group to the sample rotations [m][4] at parameters u [m]:
 *   minimises sum_i |log(S_i^-1 X(u_i))|^2 / 2 (P3ApproximationError, BsplineSO3.hpp:121-153) over steps cp <- cp exp(delta)
 *   (LocalParameterizationSO3, :190-222), first and last control point constant, Ceres' trust-region loop restated,
 *   function / gradient tolerance 1e-10, max_iterations <= 0 = Ceres' default 50.  Host only. */
int ecal_spline_so3_refine(const double *knots /*[n_cp+4]*/, uint32_t n_cp, double *cp_quat /*[n_cp][4]*/,
                           const double *sample_quat /*[m][4]*/, const double *u /*[m]*/, uint32_t m, int max_iterations,
                           double *initial_cost /*or NULL*/, double *final_cost /*or NULL*/, int *iterations /*or NULL*/);
int ecal_spline_fit(const double *u, const double *data, uint32_t m, uint32_t dim, uint32_t n_cp, double *knots /*[n_cp+4]*/,
                    double *cp /*[n_cp][dim]*/);
int ecal_spline_eval(const double *knots, const double *cp, uint32_t n_cp, uint32_t dim, const double *u, uint32_t m,
                     double *out /*[m][dim]*/);

/* ---- text ingest: "stamp x y polarity" lines into packed records, parsed in HBM ---------------------------
 * Replaces EventStream::txt2bin (event/src/EventStream.cpp:25-67, tool event/tool/txt2bin.cpp) and the reading loop behind it
 * (event_camera_calib/test/eventCameraCalib.cpp:154-163) for a text that is resident on the device.
 *
 * Input: a byte string.  A line ends at '\n'; a last line without '\n' counts.  One record per line: four fields separated
 *   by spaces or tabs, blanks before and behind them allowed, one '\r' before the line break allowed.  Lines of blanks only
 *   are skipped.  stamp = [+-]?[0-9]+ that fits an int64; x and y = [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?; polarity = 0 or 1.
 * Conversion: base = time_base when has_time_base, else the stamp of the first record line.  t = (double)(stamp - base) *
 *   time_magnitude (one integer subtraction, one conversion, one multiplication, as the reference); x, y = the correctly
 *   rounded doubles of their decimal strings (what `is >> double` gives on glibc); the polarity byte is 0 or 1.
 * Filter, in file order: with has_end_stamp the first line whose stamp > end_stamp ends the stream (the reference's break: that
 *   line and everything behind it are dropped); a record with t < 0 is dropped (the reference's continue); then the reading rule
 *   of ecal_stream_create_from_file: kept if t >= start_time, and with has_end_time the first record with t >= end_time ends
 *   the stream.
 * The reference's last record: its loop is `while (is.good()) { is >> ...; write }`, so when the file ends in white space the
 *   last pass extracts nothing and writes the last line's values once more.  With duplicate_last != 0 and a text that ends in
 *   a blank, '\r' or '\n', the record of the last record line is emitted twice if it is emitted at all.
 *   ecal_text_default_options: duplicate_last = 1 (the reference's bytes), time_magnitude = 1e-6, no base, no end stamp, no end
 *   time, start_time = -inf.
 * Differences from the reference, deliberate:
 *   1. the reference reads tokens, so a record may span lines there; here one record is one line.
 *   2. a malformed line is an error here: ECAL_ERR_INVALID, ecal_last_error and info->first_bad_line name the line (1-based).
 *      The reference ends its loop silently on a failed read and writes a record of stale values (one record of zeros for a text
 *      without any record line).
 *   3. stamp - base outside int64 is undefined in the reference and not defended here (it wraps).
 * Where the numbers are converted: the kernel converts a decimal of at most 15 significant digits whose decimal exponent
 *   (written exponent minus fraction digits) lies in [-22, 22] — one exact IEEE operation.  A line with any other well-formed
 *   number, or of more than 128 bytes, is parsed on the host with strtoll / strtod (info->n_host_lines counts them; the text and
 *   its line table are downloaded for that, which a text without such lines never pays).
 *
 * ecal_events_from_text_dev: d_text (DEVICE, 16-byte aligned, n_bytes bytes; nothing behind n_bytes is read) into d_events
 *   (DEVICE, room for `capacity` records, file order, not sorted).  info (HOST) is filled on ECAL_OK, on ECAL_ERR_RANGE
 *   (capacity too small: info->n_events = the count needed, call again; also more than 2^32-1 lines) and on ECAL_ERR_INVALID
 *   for a malformed line (first_bad_line).  On an error the contents of d_events are undefined.  Enqueues on `stream` and waits
 *   for it: the call returns with the records in place.
 * ecal_text_count_lines_dev: *n_lines (HOST) = lines of the text; lines + 1 is an upper bound for `capacity`.  Waits for `stream`.
 * ecal_stream_create_from_text_file: the file through pinned buffers into HBM (reads overlapped with the uploads, as
 *   ecal_stream_create_from_file), parsed there, the text freed, then the stream brought into time order if it is not
 *   (ecal_stream_create's rule).  ECAL_ERR_RANGE beyond 2^32-1 events.  info may be NULL.
 * ecal_text_to_bin_file: the .bin the reference's tool would write — the records in file order, no sort. */
typedef struct ecal_text_options {
    double time_magnitude;   /* seconds per stamp unit */
    int has_time_base;       /* 0: the first record line's stamp */
    int64_t time_base;
    int has_end_stamp;
    int64_t end_stamp;
    double start_time;       /* seconds */
    int has_end_time;
    double end_time;         /* seconds */
    int duplicate_last;
} ecal_text_options;
typedef struct ecal_text_info {
    uint64_t n_lines;          /* lines of the text */
    uint64_t n_blank;          /* lines of blanks only */
    uint64_t n_events;         /* records written (the duplicated last record included), or needed */
    uint64_t n_negative;       /* record lines dropped for t < 0 */
    uint64_t n_after_end;      /* record lines from the one that ended the stream on (end stamp or end time) */
    uint64_t n_before_start;   /* record lines dropped for t < start_time */
    uint64_t n_host_lines;     /* lines parsed on the host */
    uint64_t first_bad_line;   /* 1-based number of the first malformed line, 0: none */
    int64_t time_base;         /* the base in force (0 for a text without a record line and without a given base) */
} ecal_text_info;
void ecal_text_default_options(ecal_text_options *opt);
int ecal_events_from_text_dev(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const ecal_text_options *opt,
                              uint8_t *d_events /*room for capacity records*/, uint64_t capacity, ecal_text_info *info, void *stream);
int ecal_text_count_lines_dev(ecal_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint64_t *n_lines, void *stream);
int ecal_stream_create_from_text_file(ecal_ctx *ctx, const char *path, const ecal_text_options *opt, ecal_stream **out,
                                      ecal_text_info *info);
int ecal_text_to_bin_file(ecal_ctx *ctx, const char *txt_path, const char *bin_path, const ecal_text_options *opt,
                          ecal_text_info *info);

/* ---- raw ingest: Prophesee EVT3 / EVT2 recordings into packed records, decoded in HBM -----------------------
 * A camera's .raw file, without a host converter in front.  Nothing in the reference reads these encodings: this contract is the
 * specification (eventcalib_amd/csrc/raw_events.hpp restates it for the kernels, the host decoder and the tests).
 *
 * File header (file entry points only): the maximal run of lines that begin with '%' at the start of the file, each ending at
 *   '\n'.  A line that is exactly "% end" closes the header even if more '%' lines follow.  The format is taken from the first
 *   line of one of the forms "% evt 3.0", "% evt 2.0", "% format EVT3", "% format EVT2" (the last two optionally followed by
 *   ";key=value...").  options.format other than ECAL_RAW_AUTO overrides the header; no format from either source is
 *   ECAL_ERR_INVALID.  The payload starts behind the header.  The header must end within the first MiB of the file.  The _dev entry
 *   points take the payload only, with an explicit format.
 * EVT3 payload: little-endian 16-bit words, type = bits 15..12; a trailing odd byte is ignored (info.n_trailing_bytes).
 *   0x0 ADDR_Y       y = bits 10..0 (bit 11 is ignored)
 *   0x2 ADDR_X       emits one event: x = bits 10..0, polarity = bit 11, the current y.  Changes no state.
 *   0x3 VECT_BASE_X  base_x = bits 10..0, vector polarity = bit 11
 *   0x4 VECT_12      for every set bit i of bits 11..0, ascending: an event at x = base_x + i with the vector polarity; then
 *                    base_x += 12 (base_x is held in 32 bits)
 *   0x5 VECT_8       the same with bits 7..0 and += 8 (bits 11..8 are ignored)
 *   0x6 TIME_LOW     low = bits 11..0
 *   0x8 TIME_HIGH    high = bits 11..0.  Between two consecutive TIME_HIGH words with values p then q one wrap is counted when
 *                    q < p and p - q > 2048; a smaller backward step is taken as is (time then runs backwards; a stream sorts)
 *   every other type (0x7, 0xA, 0xE, 0xF, the unassigned ones: triggers among them) is skipped and counted in info.n_other_words.
 *   Event time in microseconds: t_us = (wraps << 24) | (high << 12) | low, an int64; low is 0 until the first TIME_LOW and
 *   persists across TIME_HIGH words.  An event emitted before the first TIME_HIGH, before the first ADDR_Y, or — a vector event —
 *   before the first VECT_BASE_X is dropped and counted in info.n_no_state (a vector word without a base advances nothing).
 * EVT2 payload: little-endian 32-bit words, type = bits 31..28; 1 - 3 trailing bytes are ignored and counted.
 *   0x0 CD_OFF / 0x1 CD_ON  one event of polarity 0 / 1: low6 = bits 27..22, x = bits 21..11, y = bits 10..0
 *   0x8 TIME_HIGH           high = bits 27..0
 *   t_us = (high << 6) | low6.  There is NO wrap handling: 2^34 us are 4.7 h, a longer recording's time starts again.  Events
 *   before the first TIME_HIGH are dropped (n_no_state); other types are counted in n_other_words.
 * Conversion and filter, in file order: t = (double)(t_us - time_base) * 1e-6 (one integer subtraction, one conversion, one
 *   multiplication, as the text ingest; time_base defaults to 0, the camera's clock); x, y = the doubles of the integers; the
 *   polarity byte is 0 or 1.  With width / height non-zero an event with x >= width or y >= height is dropped (n_outside); then
 *   t < 0 is dropped (n_negative); then the reading rule of ecal_stream_create_from_file: kept if t >= start_time
 *   (else n_before_start), and with has_end_time the first event with t >= end_time ends the stream: it and every event the words
 *   behind it emit count as n_after_end and as nothing else.  No record is duplicated at the end (that was a quirk of the text
 *   tool).  n_words, n_other_words, n_trailing_bytes and n_time_wraps are those of the whole payload, wherever the stream ends.
 *
 * ecal_raw_block_words: words per decode block of this build (0 for an unknown format) — a fact for tests that place block
 *   boundaries, not a tuning knob.
 * ecal_raw_count_events_dev: *n_events (HOST) = the events the words emit before any drop: always a sufficient `capacity`.  Waits
 *   for `stream`.
 * ecal_events_from_raw_dev: d_payload (DEVICE, 16-byte aligned, n_bytes bytes; nothing behind n_bytes is read) into d_events
 *   (DEVICE, room for `capacity` records, file order, not sorted); opt->format must be ECAL_RAW_EVT2 or _EVT3.  info (HOST) is
 *   filled on ECAL_OK and on ECAL_ERR_RANGE (capacity too small: info->n_events = the count needed, call again; also more than
 *   2^32-1 emitted events).  On an error the contents of d_events are undefined.  Enqueues on `stream` and waits for it: the call
 *   returns with the records in place.
 * ecal_stream_create_from_raw_file: the header read on the host, the payload through pinned buffers into HBM (reads overlapped with
 *   the uploads), decoded there, the payload freed, then the stream brought into time order if it is not (ecal_stream_create's
 *   rule).  info may be NULL.
 * ecal_raw_to_bin_file: the same records in file order, no sort, as a .bin of the reference's layout. */
enum { ECAL_RAW_AUTO = 0, ECAL_RAW_EVT2 = 2, ECAL_RAW_EVT3 = 3 };
typedef struct ecal_raw_options {
    int format;              /* ECAL_RAW_AUTO: from the file header */
    int64_t time_base;       /* microseconds of the camera's clock */
    uint32_t width, height;  /* 0: no bound */
    double start_time;       /* seconds */
    int has_end_time;
    double end_time;         /* seconds */
} ecal_raw_options;
typedef struct ecal_raw_info {
    uint64_t n_words;          /* words of the payload */
    uint64_t n_events;         /* records written, or needed */
    uint64_t n_no_state;       /* events dropped for a missing TIME_HIGH / ADDR_Y / VECT_BASE_X */
    uint64_t n_outside;        /* events dropped for x >= width or y >= height */
    uint64_t n_negative;       /* events dropped for t < 0 */
    uint64_t n_before_start;   /* events dropped for t < start_time */
    uint64_t n_after_end;      /* events from the one that ended the stream on */
    uint64_t n_other_words;    /* words of other types (triggers, ...) */
    uint64_t n_trailing_bytes; /* bytes behind the last whole word */
    uint64_t n_time_wraps;     /* EVT3: wraps of TIME_HIGH */
    int format;                /* ECAL_RAW_EVT2 / _EVT3: the format in force */
    uint64_t header_bytes;     /* file entry points: bytes in front of the payload */
} ecal_raw_info;
void ecal_raw_default_options(ecal_raw_options *opt);
uint32_t ecal_raw_block_words(int format);
int ecal_raw_count_events_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, int format, uint64_t *n_events, void *stream);
int ecal_events_from_raw_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_raw_options *opt,
                             uint8_t *d_events /*room for capacity records*/, uint64_t capacity, ecal_raw_info *info, void *stream);
int ecal_stream_create_from_raw_file(ecal_ctx *ctx, const char *path, const ecal_raw_options *opt, ecal_stream **out,
                                     ecal_raw_info *info);
int ecal_raw_to_bin_file(ecal_ctx *ctx, const char *raw_path, const char *bin_path, const ecal_raw_options *opt, ecal_raw_info *info);

/* ---- aedat ingest: iniVation AEDAT 3.1 / 2.0 recordings into packed records, decoded in HBM ------------------
 * A DAVIS camera's .aedat file, without a host converter in front.  Nothing in the reference reads these formats and no such file
 * was at hand when this was written: the layouts are restated from the published format descriptions, and this contract is the
 * specification (eventcalib_amd/csrc/aedat_events.hpp restates it for the kernels, the host decoder and the tests).  The first real
 * recording should be checked against the vendor's own export.  AEDAT 1.0 and 3.0 are not read; AEDAT 4 (compressed packets) is not
 * read HERE — it has entry points of its own, the aedat4 ingest below; a ROS 1 bag of event arrays goes through the bag ingest.
 *
 * File header (file entry points and ecal_aedat_parse_header): the first line is "#!AER-DAT3.1\r\n" or "#!AER-DAT2.0\r\n"; any
 *   other version is ECAL_ERR_INVALID with a text that names the version.  options.format other than ECAL_AEDAT_AUTO overrides the
 *   line (which then need not be there); no version from either source is ECAL_ERR_INVALID.
 *   3.1: the header runs up to and including the line "#!END-HEADER\r\n", which must lie within the first MiB (else
 *        ECAL_ERR_INVALID); a line "#Format: <value>" whose value is not RAW is ECAL_ERR_INVALID.
 *   2.0: the header is the maximal run of header lines at the start of the file.  A header line starts with '#', reaches its '\n'
 *        within 4096 bytes and holds nothing but bytes 0x20..0x7E, '\t' and '\r' before it.  (The rule is needed because the first
 *        byte of a 2.0 record can be 0x23.)
 *   info.header_bytes = where the payload starts.  The _dev entry points take the payload only, with an explicit format.
 * AEDAT 3.1 payload: a chain of packets, each a 28-byte little-endian header followed by eventCapacity x eventSize body bytes
 *   (a 64-bit product).  NO alignment of a packet may be assumed: frame packets have arbitrary sizes.  Header, by byte offset:
 *     0 i16 eventType    2 i16 eventSource    4 i32 eventSize    8 i32 eventTSOffset    12 i32 eventTSOverflow
 *     16 i32 eventCapacity    20 i32 eventNumber    24 i32 eventValid
 *   Only packets with eventType == 1 (polarity) carry events — with options.source >= 0 only those whose eventSource is that
 *   number.  Every other packet is stepped over and counted in n_other_packets.  Every packet must have eventSize, eventCapacity,
 *   eventNumber and eventValid >= 0 and eventNumber <= eventCapacity; a packet that carries events must have eventSize == 8 and
 *   eventTSOffset == 4.  A packet that breaks a rule is ECAL_ERR_INVALID; ecal_last_error names the packet's number (0-based, over
 *   all packets) and its byte offset in the payload.
 *   A polarity event is a u32 `data` followed by an i32 `ts`: bit 0 of data = valid, bit 1 = polarity, y = bits 16..2,
 *   x = bits 31..17; t_us = ((int64) eventTSOverflow << 31) + (ts & 0x7FFFFFFF).  The first eventNumber events of the body are
 *   decoded (eventValid is not relied on); an event with valid == 0 is dropped and counted in n_invalid.
 *   A header or a body that runs past the end of the payload ends the chain.  Of a body cut short the events wholly present
 *   (and in front of eventNumber) are decoded.  n_trailing_bytes: for a header cut short, the bytes from its start; for a body cut
 *   short, the bytes behind its last whole record of eventSize bytes.  The packet cut short is counted as its type says.
 * AEDAT 2.0 payload: big-endian 8-byte records, u32 address then u32 ts in microseconds; 1 - 7 trailing bytes are ignored and
 *   counted.  A DVS event has bit 31 == 0 and bit 10 == 0 of the address: x = bits 21..12, y = bits 30..22, polarity = bit 11.
 *   Every other record (APS, IMU, external input) is counted in n_other_records.  Time wraps are counted over ALL records, of
 *   every type: between consecutive records with stamps p then q one wrap is counted when q < p and p - q > 2^31; a smaller
 *   backward step is taken as it is (time then runs backwards; a stream sorts).  t_us = (wraps << 32) | ts with the wraps counted up
 *   to and including the record.  n_time_wraps, n_records, n_other_records are those of the whole payload, wherever the stream ends.
 * Conversion and filter, in file order — the raw ingest's: t = (double)(t_us - time_base) * 1e-6 (one integer subtraction, one
 *   conversion, one multiplication, no contraction); x, y = the doubles of the integers; the polarity byte is 0 or 1.  With width /
 *   height non-zero an event with x >= width or y >= height is dropped (n_outside).  flip_x / flip_y give x = width - 1 - x /
 *   y = height - 1 - y, applied BEHIND the bounds test; they need width / height non-zero (else ECAL_ERR_INVALID) and default to 0.
 *   Which flips a given recorder's files need (the origin's corner differs between tools) is the caller's knowledge and is not
 *   decided here.  Then t < 0 is dropped (n_negative); then kept if t >= start_time (else n_before_start), and with has_end_time the
 *   first event with t >= end_time ends the stream: it and every event behind it count as n_after_end and as nothing else.
 *   n_events + n_invalid + n_outside + n_negative + n_before_start + n_after_end = n_raw_events = what
 *   ecal_aedat_count_events_dev returns.
 *
 * ecal_aedat_block_events: event slots (3.1) / records (2.0) per decode block of this build (0 for an unknown format) — a fact
 *   for tests that place block boundaries, not a tuning knob.
 * ecal_aedat_parse_header: data (HOST) = the first n_bytes of a file (at most the first MiB is needed).  *format on entry is the
 *   option (ECAL_AEDAT_AUTO: from the version line), on return the format in force; *header_bytes as above.  ctx may be NULL (no
 *   error text then).
 * ecal_aedat_index_packets: a HOST function over a 3.1 payload in host memory.  One entry per polarity packet that carries events by
 *   the rules above (also one of no events), in file order.  *n_packets = the count; ECAL_ERR_RANGE when it exceeds `capacity`
 *   (out holds the first `capacity`; out may be NULL with capacity 0: a count).  info (optional): n_packets, n_other_packets,
 *   n_raw_events, n_trailing_bytes.  Only the headers are read.  ctx may be NULL (no error text then).
 *   The chain is not walked on the device: a packet is found only through the header before it.
 * ecal_aedat_count_events_dev: *n_events (HOST) = the events before any drop (3.1: the table's sum; 2.0: the DVS records): always
 *   a sufficient `capacity`.  Waits for `stream`.
 * ecal_events_from_aedat_dev: d_payload (DEVICE, 16-byte aligned, n_bytes bytes; nothing behind n_bytes is read) and, for 3.1,
 *   d_packets (DEVICE, 8-byte aligned, n_packets entries as ecal_aedat_index_packets writes them; ignored for 2.0) into d_events
 *   (DEVICE, room for `capacity` records, file order, not sorted); opt->format must be ECAL_AEDAT_3_1 or _2_0; opt->source is not
 *   looked at (the table is already of one source).  A table whose packets do not lie within the payload is ECAL_ERR_INVALID
 *   (nothing outside the payload is read).  info (HOST) is filled on ECAL_OK and on ECAL_ERR_RANGE (capacity too small:
 *   info->n_events = the count needed, call again; also more than 2^32-1 events or records); n_other_packets and the 3.1
 *   n_trailing_bytes are the indexer's to report, not this call's.  On an error the contents of d_events are undefined.  Enqueues
 *   on `stream` and waits for it: the call returns with the records in place.
 * ecal_stream_create_from_aedat_file: the header read on the host, for 3.1 the packet headers read and indexed on the host (28 bytes
 *   a packet), the payload through pinned buffers into HBM (reads overlapped with the uploads), decoded there, the payload freed,
 *   then the stream brought into time order if it is not (ecal_stream_create's rule).  info may be NULL.
 * ecal_aedat_to_bin_file: the same records in file order, no sort, as a .bin of the reference's layout. */
enum { ECAL_AEDAT_AUTO = 0, ECAL_AEDAT_2_0 = 20, ECAL_AEDAT_3_1 = 31 };
typedef struct ecal_aedat_options {
    int format;              /* ECAL_AEDAT_AUTO: from the file's version line */
    int source;              /* 3.1 file forms: >= 0, only polarity packets of this eventSource; -1: of every source */
    int64_t time_base;       /* microseconds of the camera's clock */
    uint32_t width, height;  /* 0: no bound */
    int flip_x, flip_y;      /* need width / height */
    double start_time;       /* seconds */
    int has_end_time;
    double end_time;         /* seconds */
} ecal_aedat_options;
typedef struct ecal_aedat_info {
    uint64_t n_raw_events;     /* events before any drop */
    uint64_t n_events;         /* records written, or needed */
    uint64_t n_invalid;        /* 3.1: events dropped for a clear valid bit */
    uint64_t n_outside;        /* events dropped for x >= width or y >= height */
    uint64_t n_negative;       /* events dropped for t < 0 */
    uint64_t n_before_start;   /* events dropped for t < start_time */
    uint64_t n_after_end;      /* events from the one that ended the stream on */
    uint64_t n_packets;        /* 3.1: packets that carry events */
    uint64_t n_other_packets;  /* 3.1: packets stepped over (frames, IMU, special, other sources) */
    uint64_t n_records;        /* 2.0: records of the payload */
    uint64_t n_other_records;  /* 2.0: records that are no DVS event */
    uint64_t n_trailing_bytes; /* bytes behind the last whole record */
    uint64_t n_time_wraps;     /* 2.0: wraps of the 32-bit stamp */
    uint64_t header_bytes;     /* file entry points: bytes in front of the payload */
    int format;                /* ECAL_AEDAT_3_1 / _2_0: the format in force */
} ecal_aedat_info;
typedef struct ecal_aedat_packet {
    uint64_t offset_of_first_event; /* bytes from the start of the payload */
    uint32_t n_events;              /* events to decode */
    int32_t ts_overflow;            /* the packet's eventTSOverflow */
} ecal_aedat_packet;
void ecal_aedat_default_options(ecal_aedat_options *opt);
uint32_t ecal_aedat_block_events(int format);
int ecal_aedat_parse_header(ecal_ctx *ctx, const uint8_t *data, uint64_t n_bytes, int *format, uint64_t *header_bytes);
int ecal_aedat_index_packets(ecal_ctx *ctx, const uint8_t *payload_host, uint64_t n_bytes, int source, ecal_aedat_packet *out,
                             uint64_t capacity, uint64_t *n_packets, ecal_aedat_info *info);
int ecal_aedat_count_events_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_aedat_packet *d_packets,
                                uint64_t n_packets, int format, uint64_t *n_events, void *stream);
int ecal_events_from_aedat_dev(ecal_ctx *ctx, const uint8_t *d_payload, uint64_t n_bytes, const ecal_aedat_packet *d_packets,
                               uint64_t n_packets, const ecal_aedat_options *opt, uint8_t *d_events /*room for capacity records*/,
                               uint64_t capacity, ecal_aedat_info *info, void *stream);
int ecal_stream_create_from_aedat_file(ecal_ctx *ctx, const char *path, const ecal_aedat_options *opt, ecal_stream **out,
                                       ecal_aedat_info *info);
int ecal_aedat_to_bin_file(ecal_ctx *ctx, const char *aedat_path, const char *bin_path, const ecal_aedat_options *opt,
                           ecal_aedat_info *info);

/* ---- aedat4 ingest: iniVation AEDAT 4 (DV) recordings — LZ4 packets of FlatBuffers — into packed records, inflated and decoded in HBM ----
 * The .aedat4 file DV records from a DAVIS camera, without a host converter in front.  Nothing in the reference reads it, and NO real
 * AEDAT 4 file and no vendor library was at hand when this was written: the layout is restated from the published descriptions (the DV
 * file format, FlatBuffers, the LZ4 frame and block formats), and this contract is the specification
 * (eventcalib_amd/csrc/aedat4_events.hpp restates it for the kernels, the host decoder and the tests).  The first real recording has
 * to be checked against the vendor's own export: the event count, the first and last stamps, a handful of coordinates.
 * Everything is little-endian.  Every refusal's text contains the words "AEDAT 4".
 *
 * File: bytes 0..13 are "#!AER-DAT4.0\r\n" (anything else, or a file that ends before byte 18: ECAL_ERR_INVALID).  A size-prefixed
 *   FlatBuffer follows: u32 N, then N bytes, which must lie within the first MiB; its root table is IOHeader, file identifier "IOHE" at
 *   bytes 4..7 of the N bytes (else ECAL_ERR_INVALID).  Fields by id: 0 compression i32, default 0 (NONE 0, LZ4 1, LZ4_HIGH 2, ZSTD 3,
 *   ZSTD_HIGH 4); 1 dataTablePosition i64, default -1; 2 infoNode, a string of XML, not parsed.  ZSTD and ZSTD_HIGH are refused by
 *   name (record with LZ4 or without compression); any other value is refused with its number.
 *   Packets run from byte 18 + N to dataTablePosition when that is >= 0, else to the end of the file; a position in front of the
 *   first packet or behind the end of the file is ECAL_ERR_INVALID.  A packet is i32 streamID, i32 size, then `size` bytes of data;
 *   size < 0 is ECAL_ERR_INVALID naming the packet's number (0-based, over all packets) and byte offset.  A header or data that runs
 *   past the end ends the chain: a packet cut short is not decoded at all, its bytes from the header on count as n_trailing_bytes.
 *   The file data table behind the packets is not read: a recording that was never closed reads the same as a closed one.
 * Packet data: with compression NONE the packet's FlatBuffer itself; with LZ4 or LZ4_HIGH exactly ONE LZ4 frame: magic 04 22 4D 18;
 *   FLG: bits 7..6 version, must be 01; bit 5 block independence (read, not enforced: a match is held against what the frame has
 *   produced); bit 4 block checksums; bit 3 content size present; bit 2 content checksum; bit 1 must be 0; bit 0 dictionary id:
 *   refused.  BD: bits 6..4 the block maximum, 4..7 for 64 KiB, 256 KiB, 1 MiB, 4 MiB; the other bits must be 0.  Then 8 bytes of
 *   content size if flagged, one header-checksum byte, then blocks: u32 s; s == 0 is the end mark; bit 31 set = a stored block of
 *   s & 0x7FFFFFFF bytes; else an LZ4 block of s bytes; each block followed by 4 checksum bytes if flagged.  Behind the end mark 4
 *   bytes if the content checksum is flagged, and nothing else.  CHECKSUMS ARE STEPPED OVER, NOT VERIFIED.  A flagged content size
 *   that differs from what the blocks inflate to is invalid.
 *   Block: a chain of sequences.  token: high nibble = literal length, low nibble = match length - 4; a nibble of 15 is extended by
 *   bytes, each added in, up to and including the first that is not 255.  token, literal extension, literals, u16 offset, match
 *   extension.  A block's last sequence ends behind its literals (a block that ends anywhere else is invalid).  A match may reach back
 *   up to 65 535 bytes into what the FRAME has produced, earlier blocks included; it may overlap its own output: byte i of a match is
 *   the byte at match start + (i mod offset).
 *   Malformed, all ECAL_ERR_INVALID naming the packet — its index among the event packets (0-based: the table's index) and the byte
 *   offset of its data in the file: offset 0; an offset in front of the frame's first byte; literals, offset bytes or extensions that
 *   run past the block; a block that runs past the packet; a block (stored or not) that inflates beyond the block maximum; a missing
 *   end mark; bytes behind the frame; legacy (02 21 4C 18) or skippable (5x 2A 4D 18) magic; any other magic; a frame cut short.  When
 *   several packets are malformed the lowest index the refusing pass met is named.  NOTHING outside the file or outside a packet's own
 *   span of scratch is loaded or stored, whatever the bytes say.
 * Inflated packet: a size-prefixed FlatBuffer: u32 size (not relied on), u32 root offset at byte 4, identifier at bytes 8..11, which
 *   must be "EVTS".  The table is at 4 + root, its vtable at table - (i32 at table); the vtable holds u16 vtable_bytes, u16
 *   table_bytes, u16 field0, ...  vtable_bytes < 6 or field0 == 0: the packet has no events.  Else the vector is at p + (u32 at p),
 *   p = table + field0: a u32 count, then count events of 16 bytes: i64 t (microseconds, epoch time) at 0, i16 x at 8, i16 y at 10,
 *   u8 on at 12, 3 bytes of padding.  Every one of these reads and the whole vector must lie inside the inflated packet, else
 *   ECAL_ERR_INVALID as above.  No alignment of the vector is assumed; the vtable may lie on either side of the table; further fields
 *   may follow field 0.  An inflated packet of 0 bytes (a frame whose blocks are all empty) is a packet of no events.
 * The stream: the event packets are those of ONE streamID.  options.stream_id >= 0 names it (its packets must carry EVTS); -1: the
 *   indexer inflates the first packet of every stream id on the host and takes the stream whose identifier is EVTS — two such streams
 *   (a stereo recording) and none are ECAL_ERR_INVALID with the ids in the text.  Packets of every other stream (frames, IMU,
 *   triggers) are stepped over by their header alone and counted in n_other_packets.
 * Conversion and filter, in file order — the other ingests': t = (double)(t_us - time_base) * 1e-6 (one integer subtraction, one
 *   conversion, one multiplication, no contraction); x, y = the doubles of the integers; the polarity byte is on != 0.  x < 0 or
 *   y < 0 is dropped (n_outside) always; with width / height non-zero x >= width or y >= height too.  flip_x / flip_y give
 *   x = width - 1 - x / y = height - 1 - y, applied BEHIND the bounds test; they need width / height (else ECAL_ERR_INVALID).  Then
 *   t < 0 is dropped (n_negative); then kept if t >= start_time (else n_before_start), and with has_end_time the first event with
 *   t >= end_time ends the stream: it and every event behind it count as n_after_end and as nothing else.
 *   n_events + n_outside + n_negative + n_before_start + n_after_end = n_raw_events = what ecal_aedat4_count_events_dev returns.
 * Time base: stamps are epoch microseconds.  options.auto_time_base (default 1, file forms): the base is the first event's stamp, in
 *   file order, rounded down to a whole second (0 when there is no event); the indexer reports that value as first_stamp_us.  With
 *   auto_time_base == 0 options.time_base is taken.  info.time_base = the base in force.  The _dev form takes an explicit base only:
 *   auto_time_base != 0 there is ECAL_ERR_INVALID.
 * options.max_inflated_bytes caps the sum of the packets' inflated sizes (default 2^34 = 16 GiB; an LZ4 block cannot inflate more
 *   than 255-fold, so 255 x the file is always enough): a total above it is ECAL_ERR_RANGE and the scratch for it is not allocated.
 *
 * ecal_aedat4_block_events: event slots per decode block of this build — a fact for tests that place block boundaries.
 * ecal_aedat4_parse_header: data (HOST) = the first n_bytes of a file of file_bytes bytes (at most the first MiB is needed) ->
 *   *compression, *packets_begin (18 + N), *packets_end.  ctx may be NULL (no error text then).
 * ecal_aedat4_index_packets: a HOST function over the whole file in host memory.  One 16-byte entry per packet of the chosen stream
 *   (also one of no events), in file order; offsets count from byte 0 of the file, so the table fits the file as it is uploaded.
 *   *n_packets = the count; ECAL_ERR_RANGE when it exceeds `capacity` (out holds the first `capacity`; out may be NULL with capacity
 *   0: a count).  info (optional): n_packets, n_other_packets, n_trailing_bytes, n_compressed_bytes, compression, stream_id,
 *   first_stamp_us.  ctx may be NULL.  The chain is not walked on the device: a packet is found only through the header before it.
 * ecal_aedat4_count_events_dev: *n_events (HOST) = the events before any drop: always a sufficient `capacity`.  It inflates and
 *   locates every packet to learn it (opt: compression and max_inflated_bytes are looked at).  Waits for `stream`.
 * ecal_events_from_aedat4_dev: d_file (DEVICE, 16-byte aligned, the whole file, n_bytes bytes; nothing behind n_bytes is read) and
 *   d_packets (DEVICE, 8-byte aligned, n_packets entries as ecal_aedat4_index_packets writes them) into d_events (DEVICE, room for
 *   `capacity` records, file order, not sorted).  opt->compression is explicit: ECAL_AEDAT4_NONE or ECAL_AEDAT4_LZ4 (_LZ4_HIGH is the
 *   same format); opt->stream_id is not looked at (the table is already a choice).  A table entry that does not lie within the file
 *   is ECAL_ERR_INVALID.  info (HOST) is filled on ECAL_OK and on ECAL_ERR_RANGE (capacity too small: info->n_events = the count
 *   needed, call again; also more than 2^32-1 events, and max_inflated_bytes); n_other_packets, n_trailing_bytes, stream_id and
 *   first_stamp_us are the indexer's to report, not this call's.  On an error the contents of d_events are undefined; the context
 *   stays usable.  Enqueues on `stream` and waits for it: the call returns with the records in place.
 * ecal_stream_create_from_aedat4_file: the header read on the host; the packet headers (8 bytes a packet) read, and the first packet
 *   of every stream id read and inflated for its identifier, on a host thread beside the chunked pinned upload of the file; inflated
 *   and decoded on the device, the file's bytes freed, then the stream brought into time order if it is not.  info may be NULL.
 * ecal_aedat4_to_bin_file: the same records in file order, no sort, as a .bin of the reference's layout. */
enum { ECAL_AEDAT4_NONE = 0, ECAL_AEDAT4_LZ4 = 1, ECAL_AEDAT4_LZ4_HIGH = 2, ECAL_AEDAT4_ZSTD = 3, ECAL_AEDAT4_ZSTD_HIGH = 4 };
typedef struct ecal_aedat4_options {
    int compression;             /* _dev forms: ECAL_AEDAT4_NONE or _LZ4, explicit; the file forms take the header's */
    int stream_id;               /* file forms and the indexer: >= 0 the stream of events, -1: found by its identifier */
    int auto_time_base;          /* 1: the base is the first event's whole second (file forms) */
    int flip_x, flip_y;          /* need width / height */
    int has_end_time;
    int64_t time_base;           /* microseconds of epoch time, with auto_time_base == 0 */
    uint32_t width, height;      /* 0: no upper bound */
    double start_time;           /* seconds */
    double end_time;             /* seconds */
    uint64_t max_inflated_bytes; /* default 2^34 */
} ecal_aedat4_options;
typedef struct ecal_aedat4_info {
    uint64_t n_raw_events;       /* events before any drop */
    uint64_t n_events;           /* records written, or needed */
    uint64_t n_outside;          /* events dropped for x < 0, y < 0, x >= width or y >= height */
    uint64_t n_negative;         /* events dropped for t < 0 */
    uint64_t n_before_start;     /* events dropped for t < start_time */
    uint64_t n_after_end;        /* events from the one that ended the stream on */
    uint64_t n_packets;          /* packets of the chosen stream (also those of no events) */
    uint64_t n_other_packets;    /* packets of other streams */
    uint64_t n_trailing_bytes;   /* bytes from the header of a packet cut short on */
    uint64_t n_compressed_bytes; /* data bytes of the chosen packets as the file has them */
    uint64_t n_inflated_bytes;   /* what they inflate to (NONE: the same) */
    int64_t first_stamp_us;      /* the first event's whole second: the automatic base */
    int64_t time_base;           /* the base in force */
    int compression;             /* the file's (file forms, indexer) or the option's (_dev) */
    int stream_id;               /* the chosen stream; -1: none (a file of no packets, the _dev forms) */
} ecal_aedat4_info;
typedef struct ecal_aedat4_packet {
    uint64_t offset_of_data;     /* bytes from byte 0 of the file */
    uint32_t n_bytes;            /* the packet's size */
    uint32_t zero;
} ecal_aedat4_packet;
void ecal_aedat4_default_options(ecal_aedat4_options *opt);
uint32_t ecal_aedat4_block_events(void);
int ecal_aedat4_parse_header(ecal_ctx *ctx, const uint8_t *data, uint64_t n_bytes, uint64_t file_bytes, int *compression,
                             uint64_t *packets_begin, uint64_t *packets_end);
int ecal_aedat4_index_packets(ecal_ctx *ctx, const uint8_t *file_host, uint64_t n_bytes, int stream_id, ecal_aedat4_packet *out,
                              uint64_t capacity, uint64_t *n_packets, ecal_aedat4_info *info);
int ecal_aedat4_count_events_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_aedat4_packet *d_packets,
                                 uint64_t n_packets, const ecal_aedat4_options *opt, uint64_t *n_events, void *stream);
int ecal_events_from_aedat4_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_aedat4_packet *d_packets,
                                uint64_t n_packets, const ecal_aedat4_options *opt, uint8_t *d_events /*room for capacity records*/,
                                uint64_t capacity, ecal_aedat4_info *info, void *stream);
int ecal_stream_create_from_aedat4_file(ecal_ctx *ctx, const char *path, const ecal_aedat4_options *opt, ecal_stream **out,
                                        ecal_aedat4_info *info);
int ecal_aedat4_to_bin_file(ecal_ctx *ctx, const char *aedat4_path, const char *bin_path, const ecal_aedat4_options *opt,
                            ecal_aedat4_info *info);

/* ---- bag ingest: ROS 1 bags (format 2.0) of dvs_msgs/EventArray messages into packed records, decoded in HBM ----
 * The file that rpg_dvs_ros records from a DAVIS camera, without a host converter in front.  Nothing in the reference reads a bag and
 * no bag was at hand when this was written: the layout is restated from the published descriptions (ROS bag format 2.0, ROS 1
 * message serialisation), and this contract is the specification (eventcalib_amd/csrc/bag_events.hpp restates it for the kernels,
 * the host decoder and the tests).  The first real bag should be checked against `rostopic echo` or a text dump: the event count,
 * the first and last stamps, a handful of coordinates.  Compressed chunks, format 1.2, ROS 2 containers and message packages of
 * another layout are refused by name.
 *
 * File: the 13 bytes "#ROSBAG V2.0\n", then a chain of records.  Any other "#ROSBAG V..." line is ECAL_ERR_INVALID with a text that
 *   names the version; a file that starts with "SQLite format 3\0" is refused by name as a ROS 2 bag, one that starts with
 *   "\x89MCAP0\r\n" as a ROS 2 / MCAP file; anything else is ECAL_ERR_INVALID.
 * Record: u32 header_len, header bytes, u32 data_len, data bytes; all integers of the format are little-endian.  A header is a run
 *   of fields: u32 field_len, then name=value — the name is ASCII up to the first '=', the value is binary.  Unknown fields are
 *   ignored.  A field that runs past its header (or has no '=') is ECAL_ERR_INVALID, and so is a header without a 1-byte `op`
 *   field.  Error texts name the record's number (0-based, over all records, inner and outer, in file order) and its byte offset in
 *   the file.  By op:
 *     0x03 bag header: its data is padding and is stepped over; index_pos, conn_count and chunk_count are not relied on.
 *     0x05 chunk: field `compression` must be "none" — bz2 or lz4 is ECAL_ERR_INVALID with a text that names the compression and
 *          says `rosbag decompress`; field `size` (u32) must equal data_len; the data is a chain of records walked in turn.  Inside
 *          a chunk only 0x02 and 0x07 are expected: any other op there is ECAL_ERR_INVALID, and so is an inner record that runs
 *          past the end of a chunk that is wholly present.
 *     0x07 connection, inside chunks and at top level: header fields `conn` (u32) and `topic`; the data is a second field list, of
 *          which `type` is read.  A connection seen again with the same id must name the same topic and type (else
 *          ECAL_ERR_INVALID).
 *     0x02 message data, inside chunks — at top level (an unchunked bag) it is accepted too: header fields `conn` (u32) and `time`
 *          (not used); the data is the serialised message.  A message whose connection is not defined in front of it is
 *          ECAL_ERR_INVALID.
 *     0x04 index data and 0x06 chunk info are stepped over: the index section is not used, and a bag that was never closed
 *          (index_pos == 0) reads the same as a closed one.
 *     Any other op is ECAL_ERR_INVALID.
 *   A record whose header or data runs past the end of the file ends the chain, like a recording cut short: of a chunk cut short
 *   the inner records wholly present are walked; a message cut short is not decoded at all (nor counted).  n_trailing_bytes = the
 *   bytes from the start of the first record (inner or outer) that is not wholly present.
 * Which messages carry events: chosen by their connection's type and topic.  Accepted types are dvs_msgs/EventArray and
 *   prophesee_event_msgs/EventArray (the same layout); with options.type non-empty that one name is accepted instead.  The md5sum is
 *   not looked at.  With options.topic non-empty only connections of that topic are chosen; with it empty all connections of an
 *   accepted type are, provided they share one topic: two or more event topics without a choice (a stereo bag) is
 *   ECAL_ERR_INVALID with a text that lists the topics.  No chosen connection at all is ECAL_ERR_INVALID with a text that lists the
 *   topics and types that are there.  Every message of another connection is counted in n_other_messages.
 * Message, by byte offset in the record's data:   0 u32 seq   4 u32 stamp.secs   8 u32 stamp.nsecs   12 u32 L   16 L bytes of
 *   frame_id   16+L u32 height   20+L u32 width   24+L u32 n   28+L n events of 13 bytes:
 *     0 u16 x   2 u16 y   4 u32 ts.secs   8 u32 ts.nsecs   12 u8 polarity
 *   28 + L + 13 n must equal the record's data_len, else ECAL_ERR_INVALID naming the message (this catches a message package of
 *   another layout).  NO alignment of anything may be assumed.
 * Conversion and filter, in file order — the raw and AEDAT ingests' with nanoseconds: t_ns = (int64) secs * 1 000 000 000 + nsecs
 *   (nsecs taken as it is, also >= 1e9); t = (double)(t_ns - time_base) * 1e-9 (one integer subtraction, one conversion, one
 *   multiplication, no contraction); x, y = the doubles of the integers; the polarity byte of the record is byte != 0.  With width /
 *   height non-zero an event with x >= width or y >= height is dropped (n_outside).  flip_x / flip_y give x = width - 1 - x /
 *   y = height - 1 - y, applied BEHIND the bounds test; they need width / height non-zero (else ECAL_ERR_INVALID).  Then t < 0 is
 *   dropped (n_negative); then kept if t >= start_time (else n_before_start), and with has_end_time the first event with
 *   t >= end_time ends the stream: it and every event behind it count as n_after_end and as nothing else.
 *   n_events + n_outside + n_negative + n_before_start + n_after_end = n_raw_events, always.
 * Time base: ROS stamps are epoch time; at 1.6e9 s a double resolves only 2.4e-7 s, so base 0 is useless.  options.auto_time_base
 *   (default 1): the base is secs * 1 000 000 000 of the first event, in file order, of the first chosen message that has events
 *   (0 when none has); the indexer reports that value as first_stamp_ns.  With auto_time_base == 0, options.time_base (int64
 *   nanoseconds) is taken.  info.time_base = the base in force.  The _dev entry point takes an explicit base only:
 *   auto_time_base != 0 there is ECAL_ERR_INVALID.
 *
 * ecal_bag_block_events: event slots per decode block of this build — a fact for tests that place block boundaries.
 * ecal_bag_index_messages: a HOST function over the file's bytes in host memory.  One 16-byte entry per chosen message (also one
 *   of no events), in file order; offsets count from byte 0 of the file.  opt (may be NULL): only topic and type are looked at.
 *   *n_messages = the count; ECAL_ERR_RANGE when it exceeds `capacity` (out holds the first `capacity`; out may be NULL with
 *   capacity 0: a count).  info (optional): n_messages, n_other_messages, n_chunks, n_connections, n_raw_events, n_trailing_bytes,
 *   msg_width, msg_height, first_stamp_ns.  ctx may be NULL (no error text then).
 *   The chain is not walked on the device: a message is found only through the record header before it.
 * ecal_bag_count_events_dev: *n_events (HOST) = the events before any drop (the table's sum): always a sufficient `capacity`.  Waits
 *   for `stream`.
 * ecal_events_from_bag_dev: d_file (DEVICE, 16-byte aligned, the whole file, n_bytes bytes; nothing behind n_bytes is read) and
 *   d_messages (DEVICE, 8-byte aligned, n_messages entries as ecal_bag_index_messages writes them) into d_events (DEVICE, room for
 *   `capacity` records, file order, not sorted).  opt->topic / type are not looked at (the table is already a choice).  A table
 *   entry that does not lie within the file is ECAL_ERR_INVALID, and nothing outside the file is loaded.  info (HOST) is filled on
 *   ECAL_OK and on ECAL_ERR_RANGE (capacity too small: info->n_events = the count needed, call again; also more than 2^32-1
 *   events: event indices are 32-bit per call, byte offsets 64-bit); n_other_messages, n_chunks, n_connections, n_trailing_bytes,
 *   msg_width / msg_height and first_stamp_ns are the indexer's to report, not this call's.  On an error the contents of d_events
 *   are undefined.  Enqueues on `stream` and waits for it: the call returns with the records in place.
 * ecal_stream_create_from_bag_file: the file through pinned buffers into HBM (reads overlapped with the uploads), the message table
 *   built on the host beside the upload from record headers only, decoded on the device, the file's bytes freed, then the stream
 *   brought into time order if it is not (ecal_stream_create's rule).  info may be NULL.
 * ecal_bag_to_bin_file: the same records in file order, no sort, as a .bin of the reference's layout. */
typedef struct ecal_bag_options {
    const char *topic;       /* NULL or "": every connection of an accepted type (they must share one topic) */
    const char *type;        /* NULL or "": dvs_msgs/EventArray and prophesee_event_msgs/EventArray */
    int auto_time_base;      /* 1: the base is the first event's whole seconds */
    int64_t time_base;       /* nanoseconds of epoch time, with auto_time_base == 0 */
    uint32_t width, height;  /* 0: no bound */
    int flip_x, flip_y;      /* need width / height */
    double start_time;       /* seconds */
    int has_end_time;
    double end_time;         /* seconds */
} ecal_bag_options;
typedef struct ecal_bag_info {
    uint64_t n_raw_events;     /* events before any drop */
    uint64_t n_events;         /* records written, or needed */
    uint64_t n_outside;        /* events dropped for x >= width or y >= height */
    uint64_t n_negative;       /* events dropped for t < 0 */
    uint64_t n_before_start;   /* events dropped for t < start_time */
    uint64_t n_after_end;      /* events from the one that ended the stream on */
    uint64_t n_messages;       /* chosen messages (also those of no events) */
    uint64_t n_other_messages; /* messages of other connections */
    uint64_t n_chunks;
    uint64_t n_connections;    /* distinct connection ids */
    uint64_t n_trailing_bytes; /* bytes from the first record that is not wholly present */
    int64_t first_stamp_ns;    /* the first event's secs * 1e9: the automatic base */
    int64_t time_base;         /* the base in force */
    uint32_t msg_width, msg_height; /* the first chosen message's own; may differ from the options */
} ecal_bag_info;
typedef struct ecal_bag_message {
    uint64_t offset_of_first_event; /* bytes from byte 0 of the file */
    uint32_t n_events;
    uint32_t reserved;              /* 0 */
} ecal_bag_message;
void ecal_bag_default_options(ecal_bag_options *opt);
uint32_t ecal_bag_block_events(void);
int ecal_bag_index_messages(ecal_ctx *ctx, const uint8_t *file_host, uint64_t n_bytes, const ecal_bag_options *opt, ecal_bag_message *out,
                            uint64_t capacity, uint64_t *n_messages, ecal_bag_info *info);
int ecal_bag_count_events_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_bag_message *d_messages,
                              uint64_t n_messages, uint64_t *n_events, void *stream);
int ecal_events_from_bag_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_bag_message *d_messages,
                             uint64_t n_messages, const ecal_bag_options *opt, uint8_t *d_events /*room for capacity records*/,
                             uint64_t capacity, ecal_bag_info *info, void *stream);
int ecal_stream_create_from_bag_file(ecal_ctx *ctx, const char *path, const ecal_bag_options *opt, ecal_stream **out, ecal_bag_info *info);
int ecal_bag_to_bin_file(ecal_ctx *ctx, const char *bag_path, const char *bin_path, const ecal_bag_options *opt, ecal_bag_info *info);

/* ---- array ingest: events held as columns (arrays, .npy files) packed into records in HBM, and records unpacked into columns ----
 * For events that are in memory already as t, x, y, p — from np.load, h5py, a vendor library's structured array, a torch pipeline —
 * and for the way back out.  New functionality: the reference reads its own .bin and text only.
 * eventcalib_amd/csrc/fields_events.hpp restates everything that decides for the kernels, the host entry points and the CPU test;
 * design/21_array_ingest.md has the reasoning.
 *
 * A field (ecal_field) is a column: element i lives at ptr + i * stride; stride is at least the type's size (else
 *   ECAL_ERR_INVALID).  NO alignment of ptr or stride is assumed: packed structured items of 13 or 14 bytes are the normal case.  The
 *   device loads touch only the 4-byte aligned words that hold at least one byte of an element i < n.  Types, little-endian:
 *   ECAL_FIELD_U8, I8, U16, I16, U32, I32, I64, F32, F64 (bool is U8).  t takes U32, I32, I64, F32 or F64; x, y and p take any of the
 *   nine.  A type that its field does not take is ECAL_ERR_INVALID with the field's name in the error text.
 * Conversion of event i, in input order:
 *   integer stamp: t = (double)((int64) ti - time_base) * time_magnitude (one integer subtraction, one conversion, one multiplication,
 *     no contraction: the other ingests' rule).  Float stamp: t = (double) tf * time_magnitude; time_base must be 0 (else
 *     ECAL_ERR_INVALID); with time_magnitude == 1.0 an F64 stamp passes bit for bit.
 *   x, y = the double of the value; float values are kept as they are (a sub-pixel stream can come back in).
 *   The polarity byte of the record is value > 0: 0 / 1, bool and -1 / +1 alike; NaN gives 0.
 * Filter — the bag ingest's, in its order:  with width / height non-zero an event with !(x >= 0 && x < width) or
 *   !(y >= 0 && y < height) is dropped (n_outside; a NaN coordinate is outside).  flip_x / flip_y give x = (double)(width - 1) - x /
 *   y = (double)(height - 1) - y, applied BEHIND the bounds test; they need width / height non-zero (else ECAL_ERR_INVALID).  Then
 *   !(t >= 0) is dropped (n_negative; a NaN stamp lands here); then with has_end_time the first event with t >= end_time ends the
 *   stream: it and every event behind it count as n_after_end and as nothing else; then kept if t >= start_time (else
 *   n_before_start).  n_events + n_outside + n_negative + n_before_start + n_after_end = n_raw_events, always.
 * ecal_fields_default_options: time_magnitude 1e-6, time_base 0, auto_time_base 0, no size, no flips, start_time 0, no end time.
 * Automatic time base (options.auto_time_base != 0; the host walk, the stream form and the file forms): the base is element 0's stamp
 *   for an integer stamp, 0 for a float stamp and for no events; info.time_base = the base in force.  The _dev form takes an explicit
 *   base only: auto_time_base != 0 there is ECAL_ERR_INVALID, as in the bag ingest.
 *
 * ecal_events_from_fields_host: the walk in plain C over HOST fields, no context, no device — the statement the kernels are held to.
 *   events (HOST, room for `capacity` records; more kept events than that: ECAL_ERR_RANGE with info->n_events = the count needed, the
 *   first `capacity` written).  err / err_cap (may be NULL / 0): the error text.
 * ecal_fields_block_events: events per block of the kernels — a fact for tests that place block boundaries.
 * ecal_events_from_fields_dev: f[4] = t, x, y, p over DEVICE memory, n events, into d_events (DEVICE, room for `capacity` records, input
 *   order, not sorted; any alignment; nothing behind capacity * 25 bytes is stored).  info (HOST) is filled on ECAL_OK and on
 *   ECAL_ERR_RANGE (capacity too small: info->n_events = the count needed).  n > 2^32-1: ECAL_ERR_RANGE.  n == 0 is valid.  An
 *   output that overlaps a field's bytes is ECAL_ERR_INVALID naming the field.  Enqueues on `stream` and waits for it.
 * ecal_stream_create_from_fields: HOST fields; the bytes the columns cover go up through pinned staging (13 bytes an event for the
 *   common layout, not 25; columns that share an item, as a structured array's, go up once) and are packed on the device; then the
 *   stream is brought into time order if it is not (ecal_stream_create's rule).  info may be NULL.
 * The reverse.  ecal_events_to_fields_dev: n records (DEVICE, any alignment) into out[4] = t, x, y, p over DEVICE memory (strides and
 *   alignment as above; only the elements' own bytes are stored).  F64 is a copy, F32 rounds to nearest.  An integer stamp is
 *   time_base + llrint(t * ticks_per_second): one multiplication, ties to even, one addition (default 1e6, base 0).  Integer x / y
 *   need an integral value within the type's range.  p is 0 / 1; with polarity_signed -1 / +1, and an unsigned type is then
 *   ECAL_ERR_INVALID.  Anything not representable (a non-finite stamp to an integer type included) is counted in
 *   info->n_unrepresentable and the call returns ECAL_ERR_RANGE; the output is then undefined.  An output that overlaps the records
 *   is ECAL_ERR_INVALID.  Waits for `stream`.  ecal_events_to_fields_host: the same over HOST memory, no context.
 * .npy files (`.npz` is not read here: Python opens it with numpy and comes in through the arrays).
 * ecal_npy_parse_header: HOST; ctx may be NULL.  bytes / n_bytes: the front of the file, the whole header at least; file_bytes: the
 *   file's size (0: n_bytes is the whole file).  Reads the magic \x93NUMPY, versions 1.0, 2.0 and 3.0 and the header dict as numpy
 *   writes it.  Accepted: a 1-D structured descr — a list of ('name', '<code') pairs, '|V<n>' padding entries and fields of other
 *   names stepped over — whose names are matched without case, t|ts|time|timestamp, x, y, p|pol|polarity, or exactly the names the
 *   options give; and a 2-D plain C-order array (N, 4) of one stamp type whose columns follow options.columns (default "txyp").
 *   Refused by name (ECAL_ERR_INVALID, the text in err and in ecal_last_error): big-endian codes, sub-array fields, object dtypes,
 *   fortran_order: True on 2-D data, a missing or duplicate field, a type its field does not take, and a payload shorter than the
 *   shape says (both sizes in the text).
 * ecal_stream_create_from_npy_file: the header on the host, the payload through pinned buffers into HBM from the data offset on, the
 *   fields pointing into the uploaded bytes, decoded in place; then time order as above.  ecal_npy_to_bin_file: the same records in
 *   file order, no sort, as a .bin.
 * ecal_stream_to_npy_file: a 25-byte record is exactly an item of the packed dtype [('t','<f8'),('x','<f8'),('y','<f8'),('p','u1')]:
 *   the file is a version 1.0 header and the stream's bytes as they are. */
enum {
    ECAL_FIELD_U8 = 0, ECAL_FIELD_I8 = 1, ECAL_FIELD_U16 = 2, ECAL_FIELD_I16 = 3, ECAL_FIELD_U32 = 4, ECAL_FIELD_I32 = 5,
    ECAL_FIELD_I64 = 6, ECAL_FIELD_F32 = 7, ECAL_FIELD_F64 = 8
};
typedef struct ecal_field {
    const void *ptr;
    int64_t stride;          /* bytes from one element to the next */
    uint32_t type;           /* ECAL_FIELD_* */
    uint32_t reserved;       /* 0 */
} ecal_field;
typedef struct ecal_fields_options {
    double time_magnitude;   /* seconds per tick */
    int64_t time_base;       /* ticks; 0 for a float stamp */
    int auto_time_base;      /* the base is element 0's stamp (not in the _dev form) */
    uint32_t width, height;  /* 0: no bound */
    int flip_x, flip_y;      /* need width / height */
    double start_time;       /* seconds */
    int has_end_time;
    double end_time;         /* seconds */
} ecal_fields_options;
typedef struct ecal_fields_info {
    uint64_t n_raw_events;   /* events before any drop */
    uint64_t n_events;       /* records written, or needed */
    uint64_t n_outside;
    uint64_t n_negative;
    uint64_t n_before_start;
    uint64_t n_after_end;
    int64_t time_base;       /* the base in force */
} ecal_fields_info;
typedef struct ecal_to_fields_options {
    double ticks_per_second;
    int64_t time_base;       /* ticks, added to an integer stamp */
    int polarity_signed;     /* -1 / +1 instead of 0 / 1 */
} ecal_to_fields_options;
typedef struct ecal_to_fields_info {
    uint64_t n_events;
    uint64_t n_unrepresentable;
} ecal_to_fields_info;
typedef struct ecal_npy_field {
    uint64_t offset;         /* of the field inside an item */
    uint32_t type;           /* ECAL_FIELD_* */
    uint32_t reserved;
} ecal_npy_field;
typedef struct ecal_npy_layout {
    uint64_t data_offset;    /* of element 0, from byte 0 of the file */
    uint64_t n_events;
    uint64_t item_stride;    /* bytes from one event to the next */
    ecal_npy_field field[4]; /* t, x, y, p */
    uint32_t version_major, version_minor;
} ecal_npy_layout;
typedef struct ecal_npy_options {
    ecal_fields_options fields;
    const char *t_name;      /* NULL or "": the aliases */
    const char *x_name;
    const char *y_name;
    const char *p_name;
    const char *columns;     /* of an (N, 4) array; NULL or "": "txyp" */
} ecal_npy_options;
void ecal_fields_default_options(ecal_fields_options *opt);
void ecal_to_fields_default_options(ecal_to_fields_options *opt);
void ecal_npy_default_options(ecal_npy_options *opt);
uint32_t ecal_fields_block_events(void);
int ecal_events_from_fields_host(const ecal_field f[4] /*t x y p*/, uint64_t n, const ecal_fields_options *opt, uint8_t *events,
                                 uint64_t capacity, ecal_fields_info *info, char *err, uint64_t err_cap);
int ecal_events_from_fields_dev(ecal_ctx *ctx, const ecal_field f[4] /*t x y p*/, uint64_t n, const ecal_fields_options *opt,
                                uint8_t *d_events /*room for capacity records*/, uint64_t capacity, ecal_fields_info *info, void *stream);
int ecal_stream_create_from_fields(ecal_ctx *ctx, const ecal_field f[4] /*HOST*/, uint64_t n, const ecal_fields_options *opt,
                                   ecal_stream **out, ecal_fields_info *info);
int ecal_events_to_fields_host(const uint8_t *events, uint64_t n, const ecal_field out[4], const ecal_to_fields_options *opt,
                               ecal_to_fields_info *info, char *err, uint64_t err_cap);
int ecal_events_to_fields_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n, const ecal_field out[4] /*t x y p*/,
                              const ecal_to_fields_options *opt, ecal_to_fields_info *info, void *stream);
int ecal_npy_parse_header(ecal_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t file_bytes, const ecal_npy_options *opt,
                          ecal_npy_layout *layout, char *err, uint64_t err_cap);
int ecal_stream_create_from_npy_file(ecal_ctx *ctx, const char *path, const ecal_npy_options *opt, ecal_stream **out, ecal_fields_info *info);
int ecal_npy_to_bin_file(ecal_ctx *ctx, const char *npy_path, const char *bin_path, const ecal_npy_options *opt, ecal_fields_info *info);
int ecal_stream_to_npy_file(ecal_ctx *ctx, const ecal_stream *s, const char *npy_path);

/* ---- pixel activity / hot pixels: a per-pixel count map, a mask, the stream without the masked pixels' events ----
 * A hot pixel fires events whatever the scene does.  Three stages, each callable on its own, and one call that chains them; all of
 * it opt-in (nothing else in this header calls it).  New functionality: the reference has no such filter.
 * eventcalib_amd/csrc/pixel_activity.hpp restates everything that decides for host and device; design/17_hot_pixels.md has the
 * reasoning, where the defaults come from and what was measured.  No default has met a real recording.
 *
 * The pixel of a record: x and y are the f64 at record offsets 8 and 16.  x is on the grid iff x >= 0 && x < width && x == floor(x)
 *   (NaN and +-inf are not; -0.0 is pixel 0), y the same with height; the pixel index is y * width + x.  An off-grid event is never
 *   counted in the map and never removed.  The polarity plane is `polarity byte != 0`, the board image's convention.
 * The rule (exact: integers and one double comparison per pixel):  c[p] = counts[0][p] + counts[1][p];  A = the non-zero c in
 *   ascending order;  Q = A[((len(A) - 1) * quantile_permille) / 1000] (integer division; A empty: Q = 0 and nothing is hot);
 *   p is hot iff c[p] >= min_count && (double) c[p] > factor * (double) Q;  mask = hot | extra_mask, 1 = remove.
 * width and height: 1 .. 4096, else ECAL_ERR_INVALID.  More than 2^32-1 events: ECAL_ERR_RANGE.  n_events == 0 is valid.
 * The _dev calls take any device memory of the caller's: nothing behind n_events * 25 bytes of d_events is loaded, nothing behind the
 *   kept records is stored.  They zero their outputs on `stream`, enqueue and do not synchronise.
 * ecal_pixel_activity_dev: d_counts [2][height][width] u32 (plane 0: polarity byte == 0), zeroed by the call; d_totals may be NULL.
 *   Integer atomics only: the map does not depend on the order of arrival.
 * ecal_hot_pixel_mask: HOST arrays, no context, no device.  opt NULL: the defaults.  quantile_permille > 1000, a factor that is
 *   negative or not finite: ECAL_ERR_INVALID.  info (may be NULL): n_events / n_removed / n_kept speak of the counted (on-grid)
 *   events alone and n_off_grid is 0; n_active_pixels = len(A), n_hot_pixels by the rule alone, n_masked_pixels with extra_mask,
 *   quantile_count = Q, max_count = max c, max_kept_count = max c over the pixels that are not masked.
 * ecal_filter_events_dev: the records whose pixel is not masked (d_mask [height * width] u8 on the DEVICE, non-zero = remove), their
 *   own 25 bytes each, in input order, into d_out (room for n_events records, not overlapping d_events): a time-sorted stream
 *   stays time-sorted and equal stamps keep their order.  *d_count = the records written; d_totals may be NULL;
 *   n_events = n_removed + n_kept.
 * ecal_stream_remove_hot_pixels: counts -> download -> rule -> mask upload -> filter -> a new stream (*out; `in` is untouched), on the
 *   context's stream; waits for it.  opt NULL: the defaults.  extra_mask (HOST, [height * width], may be NULL): pixels to remove
 *   whatever they count.  mask_out [height * width] and counts_out [2][height][width] (HOST, may be NULL) receive the mask and the
 *   map.  info (may be NULL): the event fields are the filter's totals (off-grid events included in n_events and n_kept). */
typedef struct ecal_activity_totals { uint64_t n_events, n_on_grid, n_off_grid; } ecal_activity_totals;
typedef struct ecal_filter_totals { uint64_t n_events, n_off_grid, n_removed, n_kept; } ecal_filter_totals;
typedef struct ecal_hot_pixel_options {
    uint32_t width, height, quantile_permille, min_count;
    double factor;
} ecal_hot_pixel_options;
typedef struct ecal_hot_pixel_info {
    uint64_t n_events, n_off_grid, n_removed, n_kept;
    uint32_t n_active_pixels, n_hot_pixels, n_masked_pixels, quantile_count, max_count, max_kept_count;
} ecal_hot_pixel_info;
void ecal_hot_pixel_default_options(ecal_hot_pixel_options *opt); /* 346 x 260, 990, 64, 8.0 */
int ecal_pixel_activity_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, uint32_t width, uint32_t height,
                            uint32_t *d_counts /*[2][H][W]; zeroed by the call*/, ecal_activity_totals *d_totals /*or NULL*/, void *stream);
int ecal_hot_pixel_mask(const uint32_t *counts /*HOST*/, const ecal_hot_pixel_options *opt, const uint8_t *extra_mask /*[H*W] or NULL*/,
                        uint8_t *mask /*[H*W], 1 = remove*/, ecal_hot_pixel_info *info);
int ecal_filter_events_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const uint8_t *d_mask, uint32_t width, uint32_t height,
                           uint8_t *d_out /*room for n_events records, not overlapping*/, uint32_t *d_count, ecal_filter_totals *d_totals,
                           void *stream);
int ecal_stream_remove_hot_pixels(ecal_ctx *ctx, const ecal_stream *in, const ecal_hot_pixel_options *opt, const uint8_t *extra_mask,
                                  ecal_stream **out, uint8_t *mask_out /*or NULL*/, uint32_t *counts_out /*or NULL*/,
                                  ecal_hot_pixel_info *info);

/* ---- noise filter: the stream without the events that have no recent neighbour event (background activity) ----
 * Background activity is isolated events spread over the whole array, with no neighbour firing near them in time.  The classic
 * filter for it, stated so that it is exact, sequentially defined and reproducible in parallel; opt-in (nothing else in this header
 * calls it).  New functionality: the reference has no such filter.  eventcalib_amd/csrc/noise_filter.hpp restates everything that
 * decides for host and device; design/19_noise_filter.md has the reasoning, where the defaults come from and what was measured.
 * The defaults come from the project's clean synthetic streams: no default has met a real recording.
 *
 * The rule: a walk over the records in stream order with a per-pixel `last` stamp and a `seen` flag, both empty at the start.  The
 *   pixel of a record and "on the grid" are the hot-pixel section's.  An off-grid event is kept, updates nothing and supports nothing.
 *   For an on-grid event i at pixel (X, Y) with stamp t_i (the f64 at record offset 0):
 *     support = the number of pixels q in the square |dx| <= radius, |dy| <= radius around (X, Y), clipped to the sensor — the own
 *       pixel only when include_self —, with seen[q] set and (t_i - last[q]) <= dt true in IEEE f64 (a NaN on either side: false);
 *     event i is kept iff support >= min_support;
 *     then last[(X, Y)] = t_i and seen[(X, Y)] = 1, whether event i was kept or not.
 *   Support is polarity-blind.  "Earlier" means earlier in the stream: events with equal stamps support one another in file order,
 *   and in an unsorted stream the most recent earlier event at q BY INDEX counts.  The first events of a stream have nothing before
 *   them and are removed.  A lone hot pixel's events are removed when include_self == 0, but a hot pixel supports its neighbours'
 *   noise: remove hot pixels first, then run this filter.
 * Options: width, height 1 .. 4096; radius 1 .. 3; min_support >= 1; include_self 0 or 1; reserved 0; dt >= 0 and not NaN (+inf is
 *   allowed), in the stream's own time unit — every ingest of this library produces seconds.  Anything else: ECAL_ERR_INVALID, and
 *   ecal_last_error names the field.  opt NULL: the defaults.  More than 2^32-1 events: ECAL_ERR_RANGE.  n_events == 0 is valid.
 * ecal_noise_verdict_host: HOST arrays, no context, no device: the walk as it is stated.  verdict [n_events]: 1 keep, 0 remove;
 *   totals may be NULL; n_events = n_removed + n_kept, the off-grid events are among the kept.
 * The _dev calls take any device memory of the caller's, whatever its alignment: nothing behind n_events * 25 bytes of d_events is
 *   loaded, nothing behind n_events verdict bytes or the kept records is stored.  They zero their outputs on `stream`, enqueue and do
 *   not synchronise.  The verdict depends on the input alone: every event is judged independently from an index of the stream by
 *   pixel (a stable radix sort), byte for byte what the walk gives.
 * ecal_noise_verdict_dev: d_verdict [n_events] u8; d_totals may be NULL.
 * ecal_denoise_events_dev: the kept records, their own 25 bytes each, in input order into d_out (room for n_events records, not
 *   overlapping d_events: ECAL_ERR_INVALID): a time-sorted stream stays time-sorted.  *d_count = the records written.
 * ecal_stream_remove_noise: a new stream (*out; `in` is untouched) on the context's stream; waits for it.  totals (HOST) may be NULL. */
typedef struct ecal_noise_options {
    uint32_t width, height, radius, min_support, include_self, reserved;
    double dt;
} ecal_noise_options;
void ecal_noise_default_options(ecal_noise_options *opt); /* 346 x 260, radius 1, min_support 1, include_self 0, dt 0.005 */
int ecal_noise_verdict_host(const uint8_t *events /*HOST*/, uint64_t n_events, const ecal_noise_options *opt, uint8_t *verdict /*HOST [n_events]*/,
                            ecal_filter_totals *totals /*or NULL*/);
int ecal_noise_verdict_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_noise_options *opt, uint8_t *d_verdict,
                           ecal_filter_totals *d_totals /*or NULL*/, void *stream);
int ecal_denoise_events_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_noise_options *opt,
                            uint8_t *d_out /*room for n_events records, not overlapping*/, uint32_t *d_count, ecal_filter_totals *d_totals,
                            void *stream);
int ecal_stream_remove_noise(ecal_ctx *ctx, const ecal_stream *in, const ecal_noise_options *opt, ecal_stream **out, ecal_filter_totals *totals);

/* ---- undistortion: the events, and event frames, of the ideal pinhole camera behind the solved one ----
 * Applies the camera the solver found.  Its intrinsics (fx fy cx cy k1..k5, the head of the solver's parameter vector) are the INVERSE
 * model — pixel to ideal ray is a closed-form polynomial —, so nothing is iterated.  The reference's PinholeCamera::undistortPoint
 * (core/sensor/src/PinholeCamera.cpp:97-126) and EventFrame::undistortedImage (event/src/EventFrame.cpp:38-60) are what this stands
 * for; Eigen's K.inverse() is NOT reproduced bit for bit: the rule below is this project's own statement, and parity with the
 * reference is unpinned here.  eventcalib_amd/csrc/undistort_point.hpp restates the rule for host and device;
 * design/20_undistort.md has the reasoning and what was measured.  Opt-in: nothing else in this header calls it.
 *
 * The rule, for a pixel (u, v).  Every operation is ONE IEEE f64 operation, rounded on its own: no FMA, a division is a division.
 *     x = (u - cx) / fx;   y = (v - cy) / fy
 *     r2 = x*x + y*y;  r4 = r2*r2;  r6 = r4*r2;  r8 = r6*r2;  r10 = r8*r2
 *     poly = ((((1 + k1*r2) + k2*r4) + k3*r6) + k4*r8) + k5*r10
 *     RADIAL :  c = poly;                                              valid iff poly > 0
 *     FISHEYE:  r2 > 1e-16: r = sqrt(r2), th = r*poly, c = tan(th)/r;  valid iff th >= 0 && th < 1.5707963267948966
 *               else       : c = poly;                                 valid iff poly > 0
 *     u' = fx' * (x*c) + cx';   v' = fy' * (y*c) + cy';                valid also needs u', v' finite
 *   A NaN anywhere makes the point invalid (every comparison above is false on a NaN).  tan is the one operation that is not
 *   correctly rounded: host and device agree to a few ulp of it there, bit for bit everywhere else.
 * The camera: ECAL_ERR_INVALID, and ecal_last_error (ecal_undistort_camera_error without a context) names the field, when fx, fy,
 *   fx' or fy' is not finite or is <= 0, a k is not finite, reserved != 0, or the model is neither of the two.
 * The options.  SUBPIXEL: a kept record carries u', v'.  PIXEL: X = round_half_away(u' + off_x), Y = round_half_away(v' + off_y) —
 *   std::round: trunc(a) + (|a - trunc(a)| >= 0.5) * sign(a), not rint and not floor(a + 0.5) —; the event is kept iff
 *   0 <= X < out_width && 0 <= Y < out_height, and its record carries X, Y as f64.  out_width, out_height 1 .. 8192, finite offsets,
 *   reserved 0 (PIXEL); an unknown mode or a non-zero reserved word: ECAL_ERR_INVALID, the field named.  opt NULL: SUBPIXEL.
 *   ecal_undistort_reference_canvas: the reference's (EventFrame.cpp:39,48-49): out = round(1.2 * size), off = size * 0.1 as f64
 *   products: 346 x 260 -> 415 x 312, off 34.6, 26.0.
 * The stream form: an invalid event is removed, in PIXEL mode one outside the canvas too.  A kept record keeps its stamp's 8 bytes and
 *   its polarity byte, whatever their values; the order of the stream is kept.  n_events = n_invalid + n_outside + n_kept.
 * ecal_undistort_points_host: HOST arrays, no context, no device.  uv [n][2] -> out [n][2] (0, 0 where invalid), flag [n]: 0 valid,
 *   1 invalid.
 * ecal_undistort_points_dev: the same per record of a packed stream (x, y at byte offsets 8 and 16 of each 25-byte record).
 * ecal_undistort_events_dev: ecal_filter_events_dev's contract — any alignment of d_events, nothing read behind n_events * 25 bytes,
 *   nothing stored behind the kept records, d_out has room for n_events records and does not overlap d_events (ECAL_ERR_INVALID), the
 *   call zeroes its outputs on `stream`, enqueues and does not synchronise; n_events == 0 is valid; more than 2^32-1 events is
 *   ECAL_ERR_RANGE.  d_totals may be NULL.
 * ecal_stream_undistort: a new stream (*out; `in` is untouched) on the context's stream; waits for it.  totals (HOST) may be NULL.
 * ecal_undistorted_frames_dev: EventFrame::undistortedImage for S windows at once, from the slicer's outputs (segment 2s the
 *   positive, 2s + 1 the negative points of window s, the pixels present in both already erased); pk NULL: every segment is doubles,
 *   else a segment is read in the form it has.  Requires opt->mode == ECAL_UNDISTORT_PIXEL.  A canvas pixel of window s is (0,255,0)
 *   if any valid negative point of the window rounds onto it, else (255,0,0) if any valid positive point does, else (0,0,0): the
 *   reference's red, then green painted over it, in RGB byte order.  Points that are invalid or land outside the canvas are counted and
 *   painted nowhere (the reference indexes out of bounds there).  d_frame_totals [S] (or NULL): n_pos / n_neg the painted points of
 *   either polarity; the four add up to the window's points.  Does not synchronise.
 * ecal_stream_undistorted_frames: window bounds, the slicer and the frames for S windows [t0[s], t1[s]] on context scratch; rgb and
 *   totals are HOST arrays; waits. */
#define ECAL_UNDISTORT_SUBPIXEL 0
#define ECAL_UNDISTORT_PIXEL 1
typedef struct ecal_undistort_camera {
    int model;         /* ECAL_CAMERA_RADIAL | ECAL_CAMERA_FISHEYE */
    int reserved;      /* 0 */
    double intr[9];    /* fx fy cx cy k1..k5: the solver's parameter head */
    double out_k[4];   /* fx' fy' cx' cy' of the ideal pinhole camera the result is expressed in */
} ecal_undistort_camera;
typedef struct ecal_undistort_options {
    uint32_t mode;             /* ECAL_UNDISTORT_SUBPIXEL 0 | ECAL_UNDISTORT_PIXEL 1 */
    uint32_t out_width, out_height;   /* PIXEL: the canvas, 1 .. 8192 */
    uint32_t reserved;
    double off_x, off_y;       /* PIXEL: added before rounding */
} ecal_undistort_options;
typedef struct ecal_undistort_totals { uint64_t n_events, n_invalid, n_outside, n_kept; } ecal_undistort_totals;
typedef struct ecal_undistort_frame_totals { uint32_t n_pos, n_neg, n_invalid, n_outside; } ecal_undistort_frame_totals;
void ecal_undistort_camera_from_params(int model, const double *params9, ecal_undistort_camera *cam); /* out_k = intr[0..3], as the reference's K_ * Xc */
void ecal_undistort_reference_canvas(uint32_t width, uint32_t height, ecal_undistort_options *opt);
/* NULL: fine; else the text that names the refused field (a static string) */
const char *ecal_undistort_camera_error(const ecal_undistort_camera *cam);
const char *ecal_undistort_options_error(const ecal_undistort_options *opt);
double ecal_undistort_round_half_away(double a);
int ecal_undistort_points_host(const ecal_undistort_camera *cam, const double *uv /*HOST [n][2]*/, uint64_t n, double *out /*HOST [n][2]*/,
                               uint8_t *flag /*HOST [n]*/);
int ecal_undistort_points_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, const uint8_t *d_events, uint64_t n_events,
                              double *d_uv /*[n][2]*/, uint8_t *d_flag /*[n]*/, void *stream);
int ecal_undistort_events_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, const ecal_undistort_options *opt, const uint8_t *d_events,
                              uint64_t n_events, uint8_t *d_out /*room for n_events records, not overlapping*/, uint32_t *d_count,
                              ecal_undistort_totals *d_totals /*or NULL*/, void *stream);
int ecal_stream_undistort(ecal_ctx *ctx, const ecal_stream *in, const ecal_undistort_camera *cam, const ecal_undistort_options *opt,
                          ecal_stream **out, ecal_undistort_totals *totals /*or NULL*/);
int ecal_undistorted_frames_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, const ecal_undistort_options *opt, const double *d_xy,
                                const ecal_packed_points *pk /*or NULL*/, const uint32_t *d_seg_off /*[2S]*/, const uint32_t *d_seg_cnt /*[2S]*/,
                                uint32_t S, uint8_t *d_rgb /*[S][out_height][out_width][3]*/,
                                ecal_undistort_frame_totals *d_frame_totals /*[S], or NULL*/, void *stream);
int ecal_stream_undistorted_frames(ecal_ctx *ctx, const ecal_stream *es, const ecal_undistort_camera *cam, const ecal_undistort_options *opt,
                                   const double *t0, const double *t1, uint32_t S, uint8_t *rgb /*HOST*/,
                                   ecal_undistort_frame_totals *totals /*HOST [S], or NULL*/);

/* ---- image undistortion: u8 frames on the ideal pinhole camera's canvas, rectification maps, the forward projection ----
 * Applies the solved camera (ecal_undistort_camera, as above; ud_point is the rule of the "undistortion" section) to pictures taken
 * through the same lens: batches of interleaved u8 frames [N][H][W][C], C = 1 or 3.  Two methods.  REFERENCE is the reference's
 * PinholeCamera::undistortImage (core/sensor/src/PinholeCamera.cpp:128-214): every source pixel is carried to the canvas, and a canvas
 * pixel is the inverse-squared-distance average of the carried pixels within 2 px of it.  BILINEAR goes the other way: the forward
 * projection (ideal pixel -> sensor pixel) gives cv::initUndistortRectifyMap's CV_32FC1 maps for the new camera out_k shifted by the
 * offsets, ready for cv::remap, and a canvas pixel is the bilinear sample of the source there.  OpenCV's own float paths (cv::Mat
 * arithmetic, cv::normalize, cv::remap's fixed-point interpolation) are NOT reproduced bit for bit: parity unpinned, as for the other
 * OpenCV calls.  eventcalib_amd/csrc/image_undistort.hpp restates the rules for host and device; design/22_image_undistort.md has the
 * reasoning and what was measured.  Opt-in: nothing else in this header calls it.  Every operation below is ONE IEEE f64 or f32
 * operation, rounded on its own: no FMA.  tan (ud_point) and atan (FISHEYE only) are the operations that are not correctly rounded.
 *
 * The options: method ECAL_IMAGE_REFERENCE | ECAL_IMAGE_BILINEAR, channels 1 | 3, out_width / out_height 1 .. 8192, normalize 0 | 1,
 *   reserved 0, finite offsets; else ECAL_ERR_INVALID with the field named (ecal_image_options_error without a context; a NULL
 *   options pointer is refused too).  The sensor: width, height 1 .. 8192.  ecal_image_reference_options: the reference's canvas
 *   (PinholeCamera.cpp:132-135): out = round_half_away(1.2 * size), off = round_half_away(size * 0.1) — ROUNDED, unlike the event
 *   frames' —, 3 channels, normalize 1, REFERENCE: 346 x 260 -> 415 x 312, off 35, 26.
 *
 * REFERENCE.  Source pixel idx = row * W + col stands at (cu, cv) = ud_point(cam, col, row) + (off_x, off_y); an invalid source pixel
 *   takes part nowhere (n_invalid_sources), and so does one with floor(cu) outside -2 .. out_width + 1 or floor(cv) outside
 *   -2 .. out_height + 1 (it neighbours nothing).  Canvas pixel (j, i) takes every source pixel with
 *       dx = j - cu;  dy = i - cv;  d2 = dx*dx + dy*dy;   d2 < 4.0   (strict: nanoflann's radius result set, squared L2)
 *       w = 1.0 / max(d2, 100 * DBL_EPSILON)
 *   in the order ascending (floor(cv), floor(cu), idx) — the reference's is its kd-tree's traversal (sorted = false), which cannot
 *   be pinned.  Per channel, over the neighbours in that order:  acc_f32 = acc_f32 + (float)(w * (double) v);  wsum_f64 = wsum_f64 + w;
 *   then avg = (float)((double) acc * (1.0 / wsum)), and 0 for a pixel without a neighbour (n_empty).
 * To u8, both methods.  normalize 1 is cv::normalize(NORM_MINMAX, 0 .. 255) over all channels and pixels of ONE frame, empty ones
 *   included:  span = (double) max - (double) min;  scale = span > DBL_EPSILON ? 255.0 / span : 0.0;
 *   out = (u8) rint((double) val * scale - (double) min * scale), ties to even.  normalize 0: out = (u8) round_half_away(val).  Both
 *   saturate at 0 and 255.
 *
 * The forward projection.  With s = r*r, s2 = s*s, s3 = s2*s, s4 = s3*s, s5 = s4*s:
 *       poly(s) = ((((1 + k1*s) + k2*s2) + k3*s3) + k4*s4) + k5*s5
 *       dp(s)   = (((k1 + (2*k2)*s) + (3*k3)*s2) + (4*k4)*s3) + (5*k5)*s4
 *       g(r)    = r * poly(r*r);      g'(r) = poly(s) + (2*s) * dp(s)
 *   The limit r_lim, once per camera and sensor on the host (ecal_camera_monotone_radius): 1.05 x the largest of
 *   sqrt(x*x + y*y), x = (u - cx) / fx, y = (v - cy) / fy over the four outer corners (-0.5 | W - 0.5, -0.5 | H - 0.5); g' is sampled at
 *   (r_lim * m) / 4096, m = 1 .. 4096, and at the first sample with !(g' > 0) r_lim falls to the sample before it and truncated = 1.
 *   A point (u', v') of the ideal camera:
 *       xu = (u' - cx') / fx';  yu = (v' - cy') / fy';  rho2 = xu*xu + yu*yu
 *       rho2 <= 1e-16: u = fx * (xu * 1) + cx,  v = fy * (yu * 1) + cy, valid, never flagged
 *       else: rho = sqrt(rho2);  T = rho (RADIAL) | atan(rho) (FISHEYE);  valid iff T <= g(r_lim)
 *             r = T * (r_lim / g(r_lim));  EIGHT times:  r = r - (g(r) - T) / g'(r);  r = r < 0 ? 0 : r;  r = r > r_lim ? r_lim : r
 *             (the count is fixed: no early exit);  ECAL_DISTORT_NOT_CONVERGED iff |g(r) - T| * max(fx, fy) > 1e-9
 *             u = fx * (xu * (r / rho)) + cx;  v = fy * (yu * (r / rho)) + cy
 *   valid also needs u, v finite; a NaN anywhere makes the point invalid (the comparisons are false on it).  flag: 0,
 *   ECAL_DISTORT_INVALID (out is 0, 0) or ECAL_DISTORT_NOT_CONVERGED (out is written all the same).
 * BILINEAR.  map_x, map_y (f32 [out_height][out_width]) and valid (u8): for canvas pixel (X, Y), (u, v) = distort(X - off_x, Y - off_y),
 *   map = ((float) u, (float) v), and (-1, -1) with valid 0 for an invalid point.  Per channel, in f32:
 *       x0 = floorf(mx);  ax = mx - x0;  y0 = floorf(my);  ay = my - y0;   a tap off the sensor is 0
 *       val = (s00*(1-ax) + s01*ax)*(1-ay) + (s10*(1-ax) + s11*ax)*ay      (s00 at (x0, y0), s01 at (x0+1, y0), s10 at (x0, y0+1))
 *
 * ecal_image_plan_create: builds the method's tables on the device, on the context's stream, and waits: REFERENCE the table of
 *   (u32 idx, f64 w) entries in the stated order with a first-entry word per canvas pixel, BILINEAR the maps.  ecal_image_plan_info:
 *   the options in force, the sensor, n_invalid_sources / n_empty (canvas pixels with no source; BILINEAR: the invalid ones) /
 *   n_entries / max_neighbours, the device bytes held, and for BILINEAR r_lim, truncated, n_invalid, n_not_converged.  A plan belongs
 *   to its context and must be destroyed before it.  ECAL_ERR_RANGE for what could hold more than 2^32-1 table entries (a source
 *   neighbours at most 13 canvas pixels: no sensor of 8192 a side gets there).
 * ecal_image_plan_maps_dev / _maps (HOST; waits): copy the maps out (any pointer may be NULL); ECAL_ERR_INVALID for a REFERENCE plan.
 * ecal_image_plan_table (HOST; waits): off [canvas pixels + 1], idx / w [n_entries]; ECAL_ERR_INVALID for a BILINEAR plan.
 * ecal_undistort_images_dev: d_src [N][H][W][C] -> d_dst [N][out_height][out_width][C]; d_minmax [N][2] f32 (or NULL): every frame's
 *   min and max of val before the rounding.  Any alignment; enqueues on `stream` and does not synchronise; N == 0 is valid; more than
 *   2^32-1 frames x canvas pixels, or more than 262140 frames, is ECAL_ERR_RANGE, before anything is launched.
 * ecal_undistort_images: the same with HOST arrays on the context's stream; waits.
 * ecal_undistort_image_host: ONE frame, HOST arrays, no context, no device: one sequential walk per method — the statement of the
 *   rule.  minmax [2] and info may be NULL (info.bytes is 0).  ecal_image_table_host / ecal_image_maps_host: the table (entries behind
 *   `capacity` are not written; info.n_entries says how many there are) and the maps of that walk.
 * ecal_distort_points_host / _dev: uv [n][2] f64 of the ideal camera -> out [n][2] (0, 0 where invalid), flag [n]. */
#define ECAL_IMAGE_REFERENCE 0
#define ECAL_IMAGE_BILINEAR 1
#define ECAL_DISTORT_INVALID 1
#define ECAL_DISTORT_NOT_CONVERGED 2
typedef struct ecal_image_options {
    uint32_t method;           /* ECAL_IMAGE_REFERENCE 0 | ECAL_IMAGE_BILINEAR 1 */
    uint32_t channels;         /* 1 | 3, interleaved u8 */
    uint32_t out_width, out_height;   /* the canvas, 1 .. 8192 */
    uint32_t normalize;        /* 1: min-max of every frame to 0 .. 255 */
    uint32_t reserved;
    double off_x, off_y;       /* canvas = ideal pixel + offset */
} ecal_image_options;
typedef struct ecal_image_info {
    ecal_image_options opt;
    uint32_t width, height;
    uint64_t n_invalid_sources, n_empty, n_entries;
    uint32_t max_neighbours, truncated;
    uint64_t bytes;
    double r_lim;
    uint64_t n_invalid, n_not_converged;
} ecal_image_info;
typedef struct ecal_image_plan ecal_image_plan;
void ecal_image_reference_options(uint32_t width, uint32_t height, ecal_image_options *opt);
const char *ecal_image_options_error(const ecal_image_options *opt);   /* NULL: fine; else the refused field (a static string) */
int ecal_camera_monotone_radius(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, double *r_lim, uint32_t *truncated);
int ecal_distort_points_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const double *uv /*HOST [n][2]*/, uint64_t n,
                             double *out /*HOST [n][2]*/, uint8_t *flag /*HOST [n]*/);
int ecal_distort_points_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const double *d_uv /*[n][2]*/,
                            uint64_t n, double *d_out /*[n][2]*/, uint8_t *d_flag /*[n]*/, void *stream);
int ecal_undistort_image_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt,
                              const uint8_t *src /*HOST [H][W][C]*/, uint8_t *dst /*HOST [oh][ow][C]*/, float *minmax /*HOST [2], or NULL*/,
                              ecal_image_info *info /*or NULL*/);
int ecal_image_table_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt,
                          uint32_t *off /*HOST [oh * ow + 1]*/, uint32_t *idx /*HOST [capacity]*/, double *w /*HOST [capacity]*/, uint64_t capacity,
                          ecal_image_info *info /*or NULL*/);
int ecal_image_maps_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt,
                         float *map_x /*HOST [oh][ow]*/, float *map_y, uint8_t *valid /*or NULL*/, ecal_image_info *info /*or NULL*/);
int ecal_image_plan_create(ecal_ctx *ctx, const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt,
                           ecal_image_plan **plan);
void ecal_image_plan_destroy(ecal_image_plan *plan);
int ecal_image_plan_info(const ecal_image_plan *plan, ecal_image_info *info);
int ecal_image_plan_maps_dev(const ecal_image_plan *plan, float *d_map_x, float *d_map_y, uint8_t *d_valid, void *stream);
int ecal_image_plan_maps(const ecal_image_plan *plan, float *map_x /*HOST*/, float *map_y /*HOST*/, uint8_t *valid /*HOST*/);
int ecal_image_plan_table(const ecal_image_plan *plan, uint32_t *off /*HOST [oh * ow + 1]*/, uint32_t *idx /*HOST [n_entries]*/,
                          double *w /*HOST [n_entries]*/);
int ecal_undistort_images_dev(ecal_ctx *ctx, const ecal_image_plan *plan, const uint8_t *d_src /*[N][H][W][C]*/, uint32_t n_frames,
                              uint8_t *d_dst /*[N][oh][ow][C]*/, float *d_minmax /*[N][2], or NULL*/, void *stream);
int ecal_undistort_images(ecal_ctx *ctx, const ecal_image_plan *plan, const uint8_t *src /*HOST*/, uint32_t n_frames, uint8_t *dst /*HOST*/,
                          float *minmax /*HOST [N][2], or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* ECAL_H_ */
