// Per-pixel event activity and the hot-pixel filter — one restatement of include/ecal.h, "pixel activity / hot pixels", for the
// kernels (ecal_activity.hip), the host rule (ecal_hot_pixel_mask) and the CPU test (tests/cpp/check_hot_pixels.cpp).
//
// Three stages.  The pixel of a record and the keep / remove verdict are per event and compile for host and device.  The rule that
// turns a count map into a mask is host code: integer arithmetic and one double comparison per pixel, no rounding that an order of
// evaluation could move.  The compaction keeps every record's own 25 bytes in input order;
//      sequential:  one walk, kept records appended
//      block-wise:  a verdict byte per event and a kept count per block, an exclusive scan of the counts, every block on its own
// give the same bytes (the kernels are the block-wise form with blocks of PA_BLOCK_EVENTS).
// design/17_hot_pixels.md has the reasoning and where the defaults come from.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_PA_HD __host__ __device__ __forceinline__
#else
#define ECAL_PA_HD inline
#endif

namespace ecal_activity {

enum : int { PA_OK = 0, PA_INVALID = -1 };   // ECAL_OK / ECAL_ERR_INVALID

constexpr uint32_t PA_RECORD_BYTES = 25;      // f64 t, f64 x, f64 y, u8 polarity (little endian, packed)
constexpr uint32_t PA_BLOCK_EVENTS = 4096;    // events per workgroup of the kernels
constexpr uint32_t PA_MAX_SIDE = 4096;        // width and height: 1 .. 4096 (a pixel index fits 24 bits)
constexpr uint32_t PA_OFF_GRID = 0xFFFFFFFFu;

// the defaults of ecal_hot_pixel_default_options
constexpr uint32_t PA_DEFAULT_WIDTH = 346, PA_DEFAULT_HEIGHT = 260, PA_DEFAULT_QUANTILE_PERMILLE = 990, PA_DEFAULT_MIN_COUNT = 64;
constexpr double PA_DEFAULT_FACTOR = 8.0;

ECAL_PA_HD double pa_load_f64(const uint8_t *p) {
    double v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// v on the grid of n cells: v >= 0, v < n, v whole.  NaN and +-inf fail the comparisons; -0.0 is cell 0.
ECAL_PA_HD bool pa_on_axis(double v, uint32_t n, uint32_t *cell) {
    if (!(v >= 0.0 && v < (double) n && v == floor(v))) return false;
    *cell = (uint32_t) v;
    return true;
}

// the pixel index y * width + x, or PA_OFF_GRID
ECAL_PA_HD uint32_t pa_pixel(double x, double y, uint32_t width, uint32_t height) {
    uint32_t xi, yi;
    if (!pa_on_axis(x, width, &xi) || !pa_on_axis(y, height, &yi)) return PA_OFF_GRID;
    return yi * width + xi;
}

ECAL_PA_HD uint32_t pa_record_pixel(const uint8_t *rec, uint32_t width, uint32_t height) {
    return pa_pixel(pa_load_f64(rec + 8), pa_load_f64(rec + 16), width, height);
}

// the polarity plane of the count map: the board image's convention
ECAL_PA_HD uint32_t pa_record_plane(const uint8_t *rec) { return rec[24] != 0 ? 1u : 0u; }

// 1: the record stays.  An off-grid event is never removed.
ECAL_PA_HD uint8_t pa_record_keep(const uint8_t *rec, const uint8_t *mask, uint32_t width, uint32_t height, bool *off_grid) {
    const uint32_t p = pa_record_pixel(rec, width, height);
    *off_grid = p == PA_OFF_GRID;
    return (uint8_t) ((p == PA_OFF_GRID || mask[p] == 0) ? 1u : 0u);
}

// ---- host: the count map ---------------------------------------------------------------------------------------------------------------
struct ActivityTotals {
    uint64_t n_events, n_on_grid, n_off_grid;
};
struct FilterTotals {
    uint64_t n_events, n_off_grid, n_removed, n_kept;
};

inline bool pa_size_ok(uint32_t width, uint32_t height) { return width >= 1 && width <= PA_MAX_SIDE && height >= 1 && height <= PA_MAX_SIDE; }

// counts [2][height][width], zeroed here
inline ActivityTotals pa_count_events(const uint8_t *rec, uint64_t n, uint32_t width, uint32_t height, uint32_t *counts) {
    const size_t plane = (size_t) width * height;
    memset(counts, 0, 2 * plane * sizeof(uint32_t));
    ActivityTotals t{n, 0, 0};
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *r = rec + i * PA_RECORD_BYTES;
        const uint32_t p = pa_record_pixel(r, width, height);
        if (p == PA_OFF_GRID) {
            t.n_off_grid++;
        } else {
            t.n_on_grid++;
            counts[pa_record_plane(r) * plane + p]++;
        }
    }
    return t;
}

// ---- host: the rule ----------------------------------------------------------------------------------------------------------------------
struct HotOptions {
    uint32_t width, height, quantile_permille, min_count;
    double factor;
};
struct HotInfo {
    uint64_t n_events, n_off_grid, n_removed, n_kept;
    uint32_t n_active_pixels, n_hot_pixels, n_masked_pixels, quantile_count, max_count, max_kept_count;
};

inline bool pa_options_ok(const HotOptions &o) {
    return pa_size_ok(o.width, o.height) && o.quantile_permille <= 1000u && o.factor >= 0.0 && o.factor <= 1.79769313486231570e308;
}

inline uint32_t pa_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) v; }

// c[p] = counts[0][p] + counts[1][p]; A = the non-zero c ascending; Q = A[((len(A) - 1) * quantile_permille) / 1000] (0 when A is
// empty: nothing is hot); p is hot iff c[p] >= min_count && (double) c[p] > factor * (double) Q; mask = hot | extra_mask (1 = remove).
// info (may be null): the event fields speak of the counted events alone (n_off_grid = 0), the u32 fields saturate.
inline int pa_hot_pixel_mask(const uint32_t *counts, const HotOptions &o, const uint8_t *extra_mask, uint8_t *mask, HotInfo *info) {
    if (!counts || !mask || !pa_options_ok(o)) return PA_INVALID;
    const size_t plane = (size_t) o.width * o.height;
    std::vector<uint64_t> A;
    A.reserve(plane);
    uint64_t c_max = 0, n_all = 0;
    for (size_t p = 0; p < plane; p++) {
        const uint64_t c = (uint64_t) counts[p] + counts[plane + p];
        if (c) A.push_back(c);
        c_max = c > c_max ? c : c_max;
        n_all += c;
    }
    uint64_t Q = 0;
    if (!A.empty()) {
        const size_t at = (size_t) (((uint64_t) (A.size() - 1) * o.quantile_permille) / 1000u);
        std::nth_element(A.begin(), A.begin() + at, A.end());
        Q = A[at];
    }
    const double bound = o.factor * (double) Q;
    uint64_t n_hot = 0, n_masked = 0, n_removed = 0, kept_max = 0;
    for (size_t p = 0; p < plane; p++) {
        const uint64_t c = (uint64_t) counts[p] + counts[plane + p];
        const bool hot = !A.empty() && c >= o.min_count && (double) c > bound;
        const bool m = hot || (extra_mask && extra_mask[p] != 0);
        mask[p] = (uint8_t) (m ? 1u : 0u);
        n_hot += hot ? 1u : 0u;
        n_masked += m ? 1u : 0u;
        if (m) n_removed += c;
        else kept_max = c > kept_max ? c : kept_max;
    }
    if (info) {
        info->n_events = n_all;
        info->n_off_grid = 0;
        info->n_removed = n_removed;
        info->n_kept = n_all - n_removed;
        info->n_active_pixels = pa_sat32(A.size());
        info->n_hot_pixels = pa_sat32(n_hot);
        info->n_masked_pixels = pa_sat32(n_masked);
        info->quantile_count = pa_sat32(Q);
        info->max_count = pa_sat32(c_max);
        info->max_kept_count = pa_sat32(kept_max);
    }
    return PA_OK;
}

// ---- host: the compaction ------------------------------------------------------------------------------------------------------------------
// out: room for n records, not overlapping rec.  Returns the totals; out holds n_kept records.
inline FilterTotals pa_filter_sequential(const uint8_t *rec, uint64_t n, const uint8_t *mask, uint32_t width, uint32_t height, uint8_t *out) {
    FilterTotals t{n, 0, 0, 0};
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *r = rec + i * PA_RECORD_BYTES;
        bool off;
        if (pa_record_keep(r, mask, width, height, &off)) {
            memcpy(out + t.n_kept * PA_RECORD_BYTES, r, PA_RECORD_BYTES);
            t.n_kept++;
        } else {
            t.n_removed++;
        }
        t.n_off_grid += off ? 1u : 0u;
    }
    return t;
}

// the kernels' three launches with blocks of `block` events: verdicts and per-block counts, the exclusive scan, every block's copy
inline FilterTotals pa_filter_blockwise(const uint8_t *rec, uint64_t n, const uint8_t *mask, uint32_t width, uint32_t height, uint32_t block,
                                        uint8_t *out) {
    FilterTotals t{n, 0, 0, 0};
    const uint64_t nb = (n + block - 1) / block;
    std::vector<uint8_t> verdict((size_t) n);
    std::vector<uint64_t> cnt((size_t) nb, 0), off((size_t) nb + 1, 0);
    for (uint64_t b = 0; b < nb; b++) {   // 1: verdicts
        const uint64_t lo = b * block, hi = lo + block < n ? lo + block : n;
        for (uint64_t i = lo; i < hi; i++) {
            bool og;
            verdict[(size_t) i] = pa_record_keep(rec + i * PA_RECORD_BYTES, mask, width, height, &og);
            cnt[(size_t) b] += verdict[(size_t) i];
            t.n_off_grid += og ? 1u : 0u;
        }
    }
    for (uint64_t b = 0; b < nb; b++) off[(size_t) b + 1] = off[(size_t) b] + cnt[(size_t) b];   // 2: scan
    for (uint64_t b = nb; b-- > 0;) {   // 3: the blocks in any order (here: backwards)
        const uint64_t lo = b * block, hi = lo + block < n ? lo + block : n;
        uint64_t at = off[(size_t) b];
        for (uint64_t i = lo; i < hi; i++)
            if (verdict[(size_t) i]) memcpy(out + (at++) * PA_RECORD_BYTES, rec + i * PA_RECORD_BYTES, PA_RECORD_BYTES);
    }
    t.n_kept = off[(size_t) nb];
    t.n_removed = n - t.n_kept;
    return t;
}
}  // namespace ecal_activity
