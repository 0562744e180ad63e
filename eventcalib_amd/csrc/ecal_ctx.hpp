// Host-side context shared by the C-ABI translation units (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include <functional>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ecal.h"

// grow-only device scratch (ecal_ensure): never shrinks, freed with its owner
struct ecal_devbuf {
    void *ptr = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return static_cast<T *>(ptr); }
    ecal_devbuf() = default;
    ecal_devbuf(const ecal_devbuf &) = delete;
    ecal_devbuf &operator=(const ecal_devbuf &) = delete;
    ~ecal_devbuf() {
        if (ptr) (void) hipFree(ptr);
    }
};
// grow-only pinned host staging (ecal_ensure_pinned): never shrinks, freed with its owner
struct ecal_pinned {
    void *ptr = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return static_cast<T *>(ptr); }
    ecal_pinned() = default;
    ecal_pinned(const ecal_pinned &) = delete;
    ecal_pinned &operator=(const ecal_pinned &) = delete;
    ~ecal_pinned() {
        if (ptr) (void) hipHostFree(ptr);
    }
};

// The scratch of the detection chain (ecal_det_slice + ecal_det_finish) for `slots` windows, sized by ecal_det_ensure (the
// whole chain) or ecal_det_ensure_bounds (the window bounds alone).  cap = cap_points + 16 points.
struct ecal_det_scratch {
    uint32_t slots = 0;                               // the windows of the last sizing call: the layout of `times`
    ecal_devbuf times;                                // [2][slots] double: every window's t0, then every window's t1
    ecal_devbuf win_lo, win_hi, win_base;             // u32 [S], [S], [S + 1]: the windows' event ranges, their points' offsets
    ecal_devbuf xy, seg_off, seg_cnt, event_point;    // the sliced points: double [cap][2], u32 [2S], u32 [2S], i32 [cap]
    ecal_devbuf labels, n_clusters, kept, rep;        // DBSCAN and the extraction: i32 [cap], u32 [2S], i32 [cap], u32 [cap]
    ecal_devbuf win_info, cand_pair, cand_xyr;        // u32 [S][4], u32 [cap][2], double [cap][3]
    ecal_devbuf overflow;                             // int: the slicer's overflow flag
    ecal_devbuf grid_order, grid_found;               // i32 [S][M], u32 [S]
    ecal_devbuf out;                                  // the entry point's result before its download (ecal_detect_pass, the tiled ingest)
    double *t0() const { return times.as<double>(); }
    double *t1() const { return times.as<double>() + slots; }
};

// Debug / test switches (ECAL_FORCE, ECAL_TRACE, ECAL_ADAPTIVE_SHAPE, …: ecal_capi.hip), read from the environment ONCE per context (ecal_init) — not per call: getenv is not safe against a
// concurrent setenv, and the entry points that consult these are the hot ones.  Tests that flip a switch on a live context call
// ecal_debug_reload_env afterwards (eventcalib_amd.capi.sync_env does it for every live context).  None of them changes a
// result, only which tier or routine produces it.
struct ecal_switches {
    // which tier / routine produces a result (parity tests run the tiers against each other)
    bool slice_no_pixel = false, dbscan_no_pixel = false, dbscan_generic_disc = false, extract_no_inline_ties = false;
    bool bounds_two_kernels = false, grid_one_wave = false, grid_serial_walk = false, solver_no_stream = false;
    int latency_forms = 0;   // ECAL_FORCE=latency_two_pass / latency_forms: 1 / 2 (ecal_latency_level)
    // traces (stderr)
    bool adaptive_trace = false, grid_debug = false, solver_trace = false, load_trace = false;
    // shape of the keyframe search's look-ahead (tests: any shape gives the same keyframes); 0 / -1: not set
    int adaptive_depth = 0, adaptive_depth_max = 0, adaptive_side = -1, adaptive_tree = -1;
    unsigned long long bo_big_arena = 0;                            // 0: not set
    double grid_tol_px = 20.0;
};
void ecal_read_switches(ecal_switches &sw);

struct ecal_ctx {
    int device = 0;
    ecal_switches sw;
    hipStream_t stream = nullptr;
    std::string last_error;
    // grow-only device scratch (never shrinks; sized for 288 GB parts: keep and reuse)
    ecal_devbuf in_xy, in_off, in_cnt, out_labels, out_ncl;  // staging for the host-pointer API
    ecal_devbuf big_slot, big_anc, big_cur, big_inv, big_cs, big_flags;    // global-scratch tier of DBSCAN
    ecal_devbuf pxs_todo;  // same for the pixel slicer
    // the insertion-order kd-trees the pixel DBSCAN kernel built (child links, 4 B per point) for the member-order kernel of the
    // exact extraction, which would otherwise build every listed segment's tree again (a third of its time): valid for the
    // labels / segment arrays of the DBSCAN call numbered px_tree_epoch, per segment when px_tree_flag[s] carries that number
    ecal_devbuf px_tree, px_tree_flag;
    uint32_t px_tree_epoch = 0, px_tree_S = 0;
    const void *px_tree_labels = nullptr, *px_tree_seg_off = nullptr;
    ecal_devbuf wb_status;  // ecal_window_bounds_dev: one word per workgroup of the look-back scan
    uint32_t wb_epoch = 0;  // ... and the number of the call that wrote it
    const uint32_t *tie_count_last = nullptr;   // the exact extraction's list counter of the last call (a zero-ring word or tie_list's own)
    const uint32_t *px_count_last[2] = {nullptr, nullptr};   // the pixel DBSCAN passes' to-do counters of the last call (zero-ring words or px_todo's own; [1] null: no second pass)
    int latency_pass = 0;             // the caller's word (the keyframe search): few of the launch's windows hold work — the stages take the forms that cost least LATENCY (1: a window through the tier it needs in one launch; 2, the search's tail: the slicer's third pass in that launch too)
    const int *overflow_sticky = nullptr;   // the caller's word: this overflow flag is zero and may STAY set once set — ecal_slice_events_dev does not wipe it (the keyframe search's passes: a memset between the kernels of a pass costs ~20 us with its gaps, and an overflow ends the search anyway)
    uint32_t grid_hint_windows = 0;   // ecal_grid_order_dev: windows that hold work in the next launch, by the caller's knowledge (0: the launch's size)
    hipStream_t wb_stream = nullptr;   // ... and the one stream whose calls use the table (others: the two-kernel form)
    bool wb_stream_set = false;
    hipEvent_t wb_done = nullptr;      // recorded behind every fused call of the owner: another stream takes the table over once it has fired
    ecal_devbuf px_todo;  // [4 + S] u32: count, then the segments the pixel kernel left to the general tiers
    ecal_devbuf sl_pts, sl_pol, sl_bend, sl_sorted, sl_rep, sl_pos;  // global-scratch tier of the slicer
    ecal_devbuf sort_scratch;  // ecal_sort_events_dev: keys, indices, radix-sort workspace
    ecal_devbuf bucket_tab;  // reference element order: bucket numbers per sensor pixel (ecal_events.hip)
    bool bucket_tab_built = false;
    ecal_devbuf sl_order, sl_order_big;  // reference element order: scratch of the general slicing tiers (slice_order.hpp)
    int point_order = ECAL_ORDER_REFERENCE;  // ecal_set_point_order
    int median_ties = ECAL_TIES_REFERENCE;   // ecal_set_median_ties: what the composite entry points do at tied medians
    ecal_devbuf det_members, det_koff, det_ksize, det_sorted, det_norms;  // detection stage scratch
    ecal_devbuf det_todo;  // [4 + S] u32: count, then the windows the first extraction pass left to the second
    ecal_devbuf tie_list, tie_order;  // ecal_extract_batch_exact_dev: windows with a tied median, their members' order
    ecal_devbuf bfs_host;   // staging of ecal_cluster_order
    ecal_devbuf bfs_lists;  // ecal_cluster_order_dev: neighbour lists of the range queries, one slice per workgroup
    ecal_devbuf bfs_defer;  // ecal_cluster_order_dev: the segments the first launch leaves to the later ones
    ecal_devbuf bfs_big;    // ecal_cluster_order_dev: workspace + hit-list arena of the global-scratch launch
    ecal_devbuf as_cnt, as_off;  // association: per-block counts / offsets
    ecal_devbuf as_host;         // staging of ecal_associate
    ecal_devbuf report_scratch;  // ecal_solver_report: the outputs' device images and the keyframe table
    ecal_devbuf board_scratch;   // ecal_solver_board_image / _board_points: the outputs' device images
    ecal_devbuf reassoc_scratch;   // ecal_solver_reassociate_dev: one verdict byte per event, per-block counts / offsets
    ecal_devbuf reassoc_records;   // ecal_solver_reassociate / _create_reassociated: the record arrays, the count, the totals
    ecal_devbuf activity_scratch;  // ecal_filter_events_dev: one verdict byte per event, per-block counts / offsets
    ecal_devbuf activity_maps;     // ecal_stream_remove_hot_pixels: the count map, the mask, the totals, the count
    ecal_devbuf noise_scratch;     // ecal_noise_verdict_dev / ecal_denoise_events_dev: sort keys and indices, sorted stamps, the start table, verdict bytes, per-block counts / offsets
    ecal_devbuf noise_results;     // ecal_stream_remove_noise: the totals, the count
    ecal_devbuf undistort_scratch; // ecal_undistort_events_dev: one verdict byte per event, per-block counts / offsets
    ecal_devbuf undistort_results; // ecal_stream_undistort: the totals, the count
    ecal_devbuf undistort_bits;    // ecal_undistorted_frames_dev: the windows' presence bits when a canvas does not fit LDS
    ecal_devbuf undistort_frames;  // ecal_stream_undistorted_frames: the pictures and the per-window totals before their download
    ecal_devbuf image_scratch;     // ecal_image_plan_create: positions, sort keys and indices, the start table, per-block counts / offsets, the counters
    ecal_devbuf image_values;      // ecal_undistort_images_dev: the frames' min / max bits, the workgroups' min / max pairs, the f32 values before their rounding to u8
    ecal_devbuf image_io;          // ecal_undistort_images: the frames, the pictures and min / max around their transfers
    ecal_devbuf aedat4_tables;    // aedat4 ingest: the packets' inflated sizes, spans, located events, first slots, the counters
    ecal_devbuf aedat4_inflated;   // aedat4 ingest: the inflated packets, each in its span (padded to 16 bytes)
    ecal_devbuf aedat4_blocks;     // aedat4 ingest: per-block kept counts / offsets
    ecal_devbuf ingest_ev[2];           // ecal_detect_stream_tiled: ping-pong event chunks
    hipStream_t copy_stream = nullptr;  // uploads of the double-buffered ingest
    ecal_pinned pass_pinned;            // ecal_detect_pass: window times in, packed verdicts out; the keyframe search: counters, report ring, handed-over frame
    ecal_pinned fetch_pinned;           // ecal_fetch_pinned: pinned staging of the larger result downloads (a hipMemcpy into pageable memory the runtime has not seen before runs at ~0.3 GB/s: 25 - 30 ms for the keyframe search's 8 MB in the first calls of a process)
    hipEvent_t ev_uploaded[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
    ecal_det_scratch det;       // the detection chain's scratch: ecal_detect_batch / _pass / _stream_tiled, the keyframe search
    ecal_devbuf host_rect[11];  // staging of ecal_rectify_batch
    ecal_devbuf calib_scratch;  // ecal_calibrate_views: views, blocks, reduced records
    ecal_devbuf adaptive_state, adaptive_keys, adaptive_dirs;  // ecal_detect_keyframes: per-piece window state, keyframe records, row directions per window
    hipEvent_t adaptive_ev[8] = {};             // ecal_detect_keyframes: one behind every pass in flight
    ecal_pinned calib_pinned;  // pinned host landing zone of the reduced record
    void *comm = nullptr;   // ncclComm_t (ecal_comm.hip); null = single rank
    int comm_rank = 0, comm_size = 1;
    // Words of device memory that are zero when handed out (ecal_zero_words): the to-do counters of the stage calls.  A ring
    // per stream that has asked (up to four), wiped half by half as it is used up.
    struct zero_ring {
        hipStream_t stream = nullptr;
        uint32_t *ptr = nullptr;
        uint32_t pos = 0;
        bool used = false;
    } zero_rings[4];
    // The later size tiers of a stage ("tails") normally find their to-do lists empty, and an empty launch still costs ~5 us:
    // 20 of them were 0.1 ms of every pass.  tail_seen = pinned host words into which the last kernel of a stage writes the
    // list counts it saw; when the stage's previous call saw empty lists (ECAL_TAIL_AUTO) the next call launches ONE tail
    // kernel that takes whatever is listed through the most general tier ("lean") instead of every tier in turn.  Either way
    // every listed window / segment is processed: the choice moves time, never results.
    uint32_t *tail_seen = nullptr, *tail_seen_dev = nullptr;   // [ECAL_TAIL_SLOTS]; 0xFFFFFFFF = not known yet
    int tail_mode = 0;                                         // ECAL_TAIL_AUTO / _TIERED / _LEAN (ecal_set_tail_mode)
    // a caller inside the library whose windows are second-tier ones by design (the keyframe search's adaptive windows): AUTO never
    // goes lean for it (the lean tail is the slow general kernel), but may still drop the tiers BEHIND the second (ecal_tail_plan)
    bool tail_no_lean = false;
    // roctx ranges around the stage entry points (ECAL_ROCTX=1 at ecal_init, or ecal_set_profile_ranges): the marker library
    // (librocprofiler-sdk-roctx.so) is looked up at run time — no link-time dependency —, `rocprofv3 --marker-trace
    // --kernel-trace` then shows which stage call every kernel belongs to (tracing)
    int (*roctx_push)(const char *) = nullptr;
    int (*roctx_pop)() = nullptr;
    void *roctx_lib = nullptr;
    uint32_t n_cu = 256;  // compute units of the device (grid size of the persistent kernels)
    bool attrs_set = false, slice_attrs_set = false, det_attr_set = false, bfs_attr_set = false;
};

#define ECAL_HIP_TRY(ctx, call)                                                                       \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess) {                                                                      \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e__);                   \
            return (e__ == hipErrorOutOfMemory) ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;                      \
        }                                                                                             \
    } while (0)

// packed points: the doubles of the listed segments / windows (ecal_events.hip)
int ecal_unpack_listed(ecal_ctx *ctx, const ecal_packed_points *pk, const uint32_t *d_list, const uint32_t *d_count, uint32_t S,
                       const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, double *d_xy, int windows, hipStream_t st);
// ecal_cluster_order_list_dev with the callers' bound on a segment's size (ecal_bfs.hip)
int ecal_cluster_order_sized(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, uint32_t S,
                             uint32_t n_points, double eps, const int32_t *d_labels, const uint32_t *d_n_clusters, int32_t *d_order,
                             uint32_t *d_status, int only_tied_medians, const uint32_t *d_win_list, const uint32_t *d_win_count,
                             void *stream, const ecal_packed_points *pk = nullptr);
// extraction as the context's ecal_set_median_ties setting wants it (ecal_detect.hip): the exact form needs the DBSCAN radius
// the pattern shapes the grid finder handles (ecal_grid.hip, next to GR_L): ECAL_OK, or ECAL_ERR_INVALID with the shape and the
// limit in ctx->last_error — every entry point that hands rows x cols to the finder asks this before it does any work
int ecal_grid_shape_check(ecal_ctx *ctx, uint32_t rows, uint32_t cols, const char *who);
// ecal_grid_order_dev + the found grids' row directions (row_direction.hpp) into d_dirs[S][rows][2] (NULL: none)
int ecal_grid_order_dirs_dev(ecal_ctx *ctx, const uint32_t *d_win_info, const uint32_t *d_seg_off, const double *d_cand_xyr, uint32_t S,
                             uint32_t rows, uint32_t cols, int32_t *d_order, uint32_t *d_found, double *d_dirs, void *stream);
int ecal_extract_for_ctx(ecal_ctx *ctx, const double *d_xy, const uint32_t *d_seg_off, const uint32_t *d_seg_cnt, const int32_t *d_labels,
                         const uint32_t *d_n_clusters, uint32_t S, uint32_t n_points, double eps, uint32_t cluster_min,
                         uint32_t need_clusters, double radius_threshold, int fit_circle, uint32_t knn_num, uint32_t *d_win_info,
                         uint32_t *d_cand_pair, double *d_cand_xyr, int32_t *d_kept_labels, uint32_t *d_rep, void *stream,
                         const ecal_packed_points *pk = nullptr);
// exclusive scan of nb per-block counts by one workgroup, off[nb] = the total (ecal_associate.hip: scan_blocks_kernel)
int ecal_scan_blocks(ecal_ctx *ctx, const uint32_t *d_cnt, uint32_t nb, uint32_t *d_off, hipStream_t st);
// an ecal_stream over device records the caller allocated (hipMalloc, n_events * 25 + 16 bytes; the stream owns them from here
// on and frees them on an error), brought into time order like ecal_stream_create's (ecal_host.hip)
int ecal_stream_adopt(ecal_ctx *ctx, uint8_t *d_events, uint64_t n_events, ecal_stream **out);
// The bytes of a file from file_offset on into a device buffer (16-byte aligned, 16 spare bytes behind; the caller's to hipFree):
// chunks read by a few threads into pinned buffers of their own, every chunk's upload enqueued as soon as it is read.  `who`
// opens the error texts.  (ecal_text.hip; the text ingest and the raw ingest)
int ecal_upload_file(ecal_ctx *ctx, const char *who, const char *path, uint64_t file_offset, uint8_t **d_out, uint64_t *n_bytes_out);
// n_events packed records on the device into the file bin_path, through pinned staging, a chunk at a time (ecal_text.hip); `prefix`
// (may be null): bytes written in front of them (the .npy header of ecal_stream_to_npy_file)
int ecal_write_records_file(ecal_ctx *ctx, const char *who, const uint8_t *d_events, uint64_t n_events, const char *bin_path,
                            const std::string *prefix = nullptr);
// ---- what the ingests' host sides share (ecal_ingest_common.hip); `who` opens the error texts ("bag ingest") -------------------------
inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }
// An argument of a device form: "<who>: null <what>" when n != 0 and ptr is null, "<who>: the <what> must be <align>-byte aligned"
// (what_aligned, when given, stands for what there), "<who>: more than 2^31-1 <plural>" when plural is given and n is above that.
int ecal_ingest_check_buffer(ecal_ctx *ctx, const char *who, const void *ptr, uint64_t n, uint32_t align, const char *what,
                             const char *what_aligned = nullptr, const char *plural = nullptr);
// an ingest's counters in front of its first kernel: zeros, and all ones in *d_none (the minimum no slot has lowered: first_stop)
int ecal_ingest_wipe_words(ecal_ctx *ctx, void *d_words, size_t bytes, unsigned long long *d_none, hipStream_t st);
// ... and on the host, behind everything enqueued on st so far
int ecal_ingest_fetch_words(ecal_ctx *ctx, void *words, const void *d_words, size_t bytes, hipStream_t st);
// The record buffer an ingest allocates for its caller: *own = room for n records (the caller's to hipFree).  ecal_ingest_drop_records
// frees it again on the way out of a failed ingest (own or *own may be null) and hands `code` through.
int ecal_ingest_alloc_records(ecal_ctx *ctx, const char *who, uint64_t n, uint8_t **own);
int ecal_ingest_drop_records(uint8_t **own, int code);
// The middle of a file form: index(&error, &table, &table_bytes) — the format's walk over the open file, on a thread of its own, which
// touches nothing of the context (null: no index, no table) — beside the upload of the file's bytes from file_offset on; fd is closed;
// the two outcomes merged (the upload's error first); "ecal <tag> ingest:" lines for the index (index_label), the upload and both
// together under ECAL_TRACE=load; the table uploaded on ctx->stream.  expect_bytes (ECAL_INGEST_ANY_SIZE: not asked): what the upload
// must have read, else "<who>: the file changed while it was read (<path>)" in front of the trace lines and the table's upload.  On success the caller ends with ecal_ingest_free_upload, which
// waits for the stream first (the table's upload reads the index's host memory); on an error nothing is left to free.
struct ecal_ingest_upload {
    uint8_t *d_file = nullptr;
    uint64_t n_bytes = 0;
    void *d_table = nullptr;
};
typedef std::function<int(std::string *error, const void **table, size_t *table_bytes)> ecal_ingest_index_fn;
constexpr uint64_t ECAL_INGEST_ANY_SIZE = ~0ull;
int ecal_ingest_upload_indexed(ecal_ctx *ctx, const char *tag, const char *who, const char *index_label, const char *path, int fd,
                               uint64_t file_offset, uint64_t expect_bytes, const ecal_ingest_index_fn &index, ecal_ingest_upload *up);
void ecal_ingest_free_upload(ecal_ctx *ctx, ecal_ingest_upload *up);
// n bytes of fd from `at` on into dst, in as many reads as it takes; false when the file ends first or a read fails
bool ecal_ingest_pread_all(int fd, void *dst, size_t n, uint64_t at);
// Bytes of a file through a small read-ahead window: a host index walk asks for a record's header, a schema, the front of a message —
// a few dozen bytes at places 10 – 100 KB apart — and one pread of a window serves the neighbours.
struct ecal_ingest_file_reader {
    int fd;
    uint64_t file_bytes;
    std::vector<uint8_t> win;
    uint64_t win_at = 0, win_n = 0;
    static constexpr size_t WINDOW = 512;
    bool operator()(uint64_t pos, uint8_t *dst, size_t n);
};
// The front of a file form: path opened (*fd), *file_bytes = its size, *head = its first min(size, head_max) bytes.  "<who>: cannot open
// <path>"; "<who>: cannot read <path>" for a size that cannot be asked and for a head that cannot be read — the latter as "<who>:
// <unread> (<path>)" where `unread` is given.  ECAL_ERR_INVALID with the file closed again.
int ecal_ingest_open_head(ecal_ctx *ctx, const char *who, const char *path, size_t head_max, const char *unread, int *fd, uint64_t *file_bytes,
                          std::vector<uint8_t> *head);
// a file form's records as a stream (d_events null: no events, a stream of none), or written to bin_path and freed
int ecal_stream_from_events(ecal_ctx *ctx, const char *who, uint8_t *d_events, uint64_t n_events, ecal_stream **out);
int ecal_ingest_records_to_bin(ecal_ctx *ctx, const char *who, uint8_t *d_events, uint64_t n_events, const char *bin_path);
// ECAL_TRACE=load: device time of an ingest's phases, "ecal <what> ingest: <phase> <ms>" lines on stderr when it goes out of scope
struct ecal_load_timer {
    const char *what;
    bool on;
    hipStream_t st;
    hipEvent_t ev[8] = {};
    const char *name[8] = {};
    int n = 0;
    ecal_load_timer(const char *what_, bool enabled, hipStream_t s) : what(what_), on(enabled), st(s) {}
    void mark(const char *phase) {
        if (!on || n >= 8) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) {
            on = false;
            return;
        }
        (void) hipEventRecord(ev[n], st);
        name[n++] = phase;
    }
    ~ecal_load_timer() {
        for (int i = 1; i < n && on; i++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i - 1], ev[i]) == hipSuccess) fprintf(stderr, "ecal %s ingest: %-24s %.3f ms\n", what, name[i], ms);
        }
        for (int i = 0; i < n; i++) (void) hipEventDestroy(ev[i]);
    }
};
// ---- what the compacting stages share on the host (ecal_activity.hip): the hot-pixel filter, the noise filter, undistortion and
// re-association judge every event of a packed stream, count the kept events per block of ECAL_STREAM_BLOCK, scan the counts and
// write the kept events out in input order (the device side: stream_compact.hpp) ---------------------------------------------------
constexpr uint32_t ECAL_STREAM_BLOCK = 4096;
// verdicts (whole blocks, 16-byte aligned) | counts [nb] | offsets [nb + 1]
struct ecal_verdict_tables {
    uint8_t *verdict;
    uint32_t *cnt, *off;
    uint32_t nb;
};
inline uint32_t ecal_stream_blocks(uint64_t n_events) { return (uint32_t) ((n_events + ECAL_STREAM_BLOCK - 1) / ECAL_STREAM_BLOCK); }
inline size_t ecal_verdict_tables_bytes(uint32_t nb) { return (size_t) nb * ECAL_STREAM_BLOCK + (size_t) nb * 4 + ((size_t) nb + 1) * 4; }
inline ecal_verdict_tables ecal_verdict_tables_at(uint8_t *base, uint32_t nb) {
    uint8_t *cnt = base + (size_t) nb * ECAL_STREAM_BLOCK;
    return ecal_verdict_tables{base, reinterpret_cast<uint32_t *>(cnt), reinterpret_cast<uint32_t *>(cnt + (size_t) nb * 4), nb};
}
// ... for n_events events in a scratch buffer of their own
int ecal_verdict_tables_ensure(ecal_ctx *ctx, ecal_devbuf &scratch, uint64_t n_events, ecal_verdict_tables *V);
// "<who>: more than 2^32-1 events" (ECAL_ERR_RANGE)
int ecal_events_range_check(ecal_ctx *ctx, const char *who, uint64_t n_events);
// A compacting _dev form behind its own null-pointer, option and range tests (their order is each entry point's): "<who>: the output
// overlaps the events" (d_out null: not asked — re-association writes other arrays), the context's device, and *d_count and the
// d_totals (may be null) zeroed
int ecal_compact_begin(ecal_ctx *ctx, const char *who, const uint8_t *d_events, uint64_t n_events, const uint8_t *d_out, uint32_t *d_count,
                       void *d_totals, size_t totals_bytes, hipStream_t st);
// The ordered compaction every one of them ends in: the exclusive scan of the per-block kept counts V.cnt into V.off, launch_write()
// — the stage's writing kernel over V.nb workgroups — and *d_count = the total.  n_events > 0.  Marks "scan" and "write" on tm (may
// be null); does not synchronise.
template <class Launch>
int ecal_compact_by_verdict(ecal_ctx *ctx, const ecal_verdict_tables &V, uint32_t *d_count, ecal_load_timer *tm, hipStream_t st,
                            Launch launch_write) {
    const int rc = ecal_scan_blocks(ctx, V.cnt, V.nb, V.off, st);
    if (rc) return rc;
    if (tm) tm->mark("scan");
    launch_write();
    if (tm) tm->mark("write");
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_count, V.off + V.nb, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}
// ... with activity_write_kernel: the events whose verdict byte is non-zero, their own 25 bytes each, into d_out (both filters)
int ecal_compact_copy_by_verdict(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_verdict_tables &V, uint8_t *d_out,
                                 uint32_t *d_count, ecal_load_timer &tm, hipStream_t st);
// The stream form of a compacting stage, on ctx->stream: records of the new stream's own (every event may stay), run_dev — the _dev
// form into them, d_results = totals (totals_bytes) | count —, the totals into `totals` and the count in ONE synchronisation, then
// disagree(kept, n): null, or what is wrong with the counters ("<who>: <that>", ECAL_ERR_HIP; it may hand the totals on first).  The
// records are dropped on every failure; the stream is synchronised before any return.
typedef std::function<int(uint8_t *d_out, uint32_t *d_count, void *d_totals, hipStream_t st)> ecal_stream_dev_fn;
typedef std::function<const char *(uint32_t kept, uint64_t n)> ecal_stream_disagree_fn;
int ecal_stream_compacted(ecal_ctx *ctx, const char *who, const ecal_stream *in, void *d_results, void *totals, size_t totals_bytes,
                          const ecal_stream_dev_fn &run_dev, const ecal_stream_disagree_fn &disagree, ecal_stream **out);
// reference element order: the per-pixel bucket table of the hot-path slicer, built on first use (ecal_events.hip)
int ecal_ensure_bucket_table(ecal_ctx *ctx, hipStream_t st);
// tail scheduling (see ecal_ctx::tail_seen): slots of the stages' lists, and "may this call run lean?"
enum { ECAL_TAIL_SLICE = 0, ECAL_TAIL_DBSCAN = 2, ECAL_TAIL_EXTRACT = 4, ECAL_TAIL_ORDER = 6, ECAL_TAIL_SLOTS = 16 };
inline bool ecal_tail_lean(const ecal_ctx *ctx, int first, int n) {
    if (ctx->tail_mode == ECAL_TAIL_LEAN) return true;
    if (ctx->tail_mode == ECAL_TAIL_TIERED || !ctx->tail_seen) return false;
    for (int k = 0; k < n; k++)
        if (__atomic_load_n(ctx->tail_seen + first + k, __ATOMIC_RELAXED) != 0u) return false;
    return true;
}
// The plan of a stage whose to-do lists sit in slots first (what the first pass listed) and first + 1 (what the second pass left
// of that): LEAN — one general launch behind the first pass; SEMI — first and second pass, then one general launch for whatever
// the second pass leaves (normally nothing: the tiers behind it are three to five launches that find their list empty); TIERED —
// every tier.  AUTO decides by what the stage's previous call on this context saw; whatever the plan, every listed window is
// processed and the results are bit-identical (tests/test_gpu_tail_modes.py).
enum { ECAL_PLAN_TIERED = 0, ECAL_PLAN_SEMI = 1, ECAL_PLAN_LEAN = 2 };
inline int ecal_tail_plan(const ecal_ctx *ctx, int first) {
    if (ctx->tail_mode == ECAL_TAIL_LEAN) return ECAL_PLAN_LEAN;
    if (ctx->tail_mode == ECAL_TAIL_TIERED || !ctx->tail_seen) return ECAL_PLAN_TIERED;
    const uint32_t a = __atomic_load_n(ctx->tail_seen + first, __ATOMIC_RELAXED), b = __atomic_load_n(ctx->tail_seen + first + 1, __ATOMIC_RELAXED);
    if (a == 0u && b == 0u && !ctx->tail_no_lean) return ECAL_PLAN_LEAN;
    if (a != 0xFFFFFFFFu && b == 0u) return ECAL_PLAN_SEMI;
    return ECAL_PLAN_TIERED;
}
// the latency forms' level of a stage call: the caller's word (ecal_ctx::latency_pass), or 1 / 2 under ECAL_FORCE=latency_two_pass /
// latency_forms (tests: the forms against the staged passes outside the keyframe search)
inline int ecal_latency_level(const ecal_ctx *ctx) { return ctx->sw.latency_forms ? ctx->sw.latency_forms : ctx->latency_pass; }
// a roctx range for the lifetime of the object (nothing when the context has no marker library loaded)
struct ecal_range {
    const ecal_ctx *c;
    ecal_range(const ecal_ctx *ctx, const char *name) : c(ctx && ctx->roctx_push ? ctx : nullptr) {
        if (c) (void) c->roctx_push(name);
    }
    ~ecal_range() {
        if (c && c->roctx_pop) (void) c->roctx_pop();
    }
    ecal_range(const ecal_range &) = delete;
    ecal_range &operator=(const ecal_range &) = delete;
};
// n <= 16 words that are zero once everything enqueued on `st` so far has run, or nullptr (more streams than rings, no memory):
// the caller then zeroes words of its own.  They stay the caller's for the next 512 calls on that stream at least.
uint32_t *ecal_zero_words(ecal_ctx *ctx, hipStream_t st, uint32_t n);
// pinned host staging of at least `bytes` (grow-only, contents NOT preserved; nullptr: no memory — the caller copies the slow way)
unsigned char *ecal_fetch_pinned(ecal_ctx *ctx, size_t bytes);
// ensure a scratch buffer of at least `bytes` (contents are NOT preserved)
int ecal_ensure(ecal_ctx *ctx, ecal_devbuf &b, size_t bytes);
// the same for pinned host staging: hipSuccess, or the allocation's error with the buffer left empty
hipError_t ecal_ensure_pinned(ecal_pinned &b, size_t bytes);
// ctx->det for S windows of up to cap_points points and M = rows x cols grid points (0: no grid stage), or for the window
// bounds alone; either sets the layout of det.times
int ecal_det_ensure(ecal_ctx *ctx, uint32_t S, uint32_t cap_points, uint32_t M);
int ecal_det_ensure_bounds(ecal_ctx *ctx, uint32_t S);
// The detection chain on ctx->det for the S windows whose times stand in det.t0() / det.t1(), over d_events[0, n_events) (ecal_host.hip).
// ecal_det_slice: window bounds, slicing.  ecal_det_finish: DBSCAN, extraction and, when prm->rows x cols > 0, the grid finder,
// with the found grids' row directions into d_dirs[S][rows][2] (null: none) and grid_hint as ecal_ctx::grid_hint_windows for
// its call.  (Two calls: the double-buffered ingest frees its event chunk between them.)
int ecal_det_slice(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, uint32_t S, uint32_t cap_points, hipStream_t st);
int ecal_det_finish(ecal_ctx *ctx, uint32_t S, const ecal_detect_params *prm, uint32_t cap_points, double *d_dirs, uint32_t grid_hint,
                    hipStream_t st);
inline int ecal_det_chain(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, uint32_t S, const ecal_detect_params *prm,
                          uint32_t cap_points, double *d_dirs, uint32_t grid_hint, hipStream_t st) {
    const int rc = ecal_det_slice(ctx, d_events, n_events, S, cap_points, st);
    return rc ? rc : ecal_det_finish(ctx, S, prm, cap_points, d_dirs, grid_hint, st);
}
