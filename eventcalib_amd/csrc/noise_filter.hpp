// The background-activity ("noise") filter — one restatement of include/ecal.h, "noise filter", for the kernels (ecal_noise.hip), the
// host entry point (ecal_noise_verdict_host) and the CPU test (tests/cpp/check_noise_filter.cpp).
//
// The rule is a sequential walk over the records in stream order with a per-pixel `last` stamp and a `seen` flag, both empty at the
// start.  An off-grid event (pixel_activity.hpp's pa_record_pixel says which) is kept, updates nothing and supports nothing.  For an
// on-grid event i at pixel (X, Y) with stamp t_i,
//      support = the number of pixels q in the square |dx| <= radius, |dy| <= radius around (X, Y), clipped to the sensor, the own
//                pixel only with include_self, with seen[q] set and (t_i - last[q]) <= dt true in IEEE f64 (a NaN on either side:
//                false; dt = +inf: every finite difference supports)
//      event i is kept iff support >= min_support
//      then last[(X, Y)] = t_i and seen[(X, Y)] = 1, whether event i was kept or not.
// What follows:
//   - support is polarity-blind;
//   - "earlier" means earlier in the STREAM: events with equal stamps support one another in file order;
//   - the rule is defined on indices, so it is well defined for an unsorted stream too: the most recent earlier event at q by index
//     is the one that counts (its stamp may lie in the future of t_i: the difference is negative and supports);
//   - the first events of a stream have nothing before them and are removed — the start-up artefact of every such filter;
//   - a lone hot pixel's events are removed when include_self == 0, but a hot pixel does support its neighbours' noise: hot pixels
//     first (pixel_activity.hpp), then this filter.
//
// The verdict depends on the input stream alone, never on earlier verdicts, so every event can be judged on its own given, for each
// neighbour pixel, the most recent earlier event there.  The indexed form (the kernels', nf_verdict_indexed on the host):
//      key[i] = the pixel of event i (off-grid: width * height), val[i] = i; a STABLE sort of the pairs by key: every pixel's events
//      form one contiguous list of ascending stream indices;  start[p] = the first sorted position with key >= p (plane + 1 words);
//      the stamps gathered into sorted order;  per sorted position, for each neighbour q a binary search of q's list for the last
//      entry with index < i (nf_last_before; the own pixel's is the position in front), one support test on its stamp.
// design/19_noise_filter.md has the reasoning and where the defaults come from.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "pixel_activity.hpp"

namespace ecal_noise {

using ecal_activity::FilterTotals;
using ecal_activity::PA_OFF_GRID;
using ecal_activity::PA_RECORD_BYTES;

constexpr uint32_t NF_MAX_RADIUS = 3;
constexpr uint32_t NF_NONE = 0xFFFFFFFFu;   // nf_last_before: no earlier event in the list

// the defaults of ecal_noise_default_options
constexpr uint32_t NF_DEFAULT_WIDTH = 346, NF_DEFAULT_HEIGHT = 260, NF_DEFAULT_RADIUS = 1, NF_DEFAULT_MIN_SUPPORT = 1, NF_DEFAULT_INCLUDE_SELF = 0;
constexpr double NF_DEFAULT_DT = 0.005;

// ecal_noise_options, field for field
struct NoiseOptions {
    uint32_t width, height, radius, min_support, include_self, reserved;
    double dt;
};

inline NoiseOptions nf_default_options() {
    return NoiseOptions{NF_DEFAULT_WIDTH, NF_DEFAULT_HEIGHT, NF_DEFAULT_RADIUS, NF_DEFAULT_MIN_SUPPORT, NF_DEFAULT_INCLUDE_SELF, 0u, NF_DEFAULT_DT};
}

// nullptr: the options are fine; else the field that is not, with its range
inline const char *nf_options_error(const NoiseOptions &o) {
    if (!ecal_activity::pa_size_ok(o.width, o.height)) return "width and height from 1 to 4096";
    if (o.radius < 1 || o.radius > NF_MAX_RADIUS) return "radius from 1 to 3";
    if (o.min_support < 1) return "min_support at least 1";
    if (o.include_self > 1) return "include_self 0 or 1";
    if (o.reserved != 0) return "reserved must be 0";
    if (!(o.dt >= 0.0)) return "dt at least 0 and not NaN";
    return nullptr;
}

// the sort key of a record: its pixel, or width * height off the grid
ECAL_PA_HD uint32_t nf_record_key(const uint8_t *rec, uint32_t width, uint32_t height) {
    const uint32_t p = ecal_activity::pa_record_pixel(rec, width, height);
    return p == PA_OFF_GRID ? width * height : p;
}

// the bits of the largest key, width * height: ceil(log2(width * height + 1)), 1 .. 25
ECAL_PA_HD uint32_t nf_key_bits(uint32_t plane) {
    uint32_t b = 1;
    while (b < 32 && (plane >> b) != 0) b++;
    return b;
}

// the square around (x, y), clipped to the sensor: [x0, x1] x [y0, y1], walked row by row
ECAL_PA_HD void nf_window(uint32_t x, uint32_t y, uint32_t radius, uint32_t width, uint32_t height, uint32_t *x0, uint32_t *x1, uint32_t *y0,
                          uint32_t *y1) {
    *x0 = x >= radius ? x - radius : 0u;
    *y0 = y >= radius ? y - radius : 0u;
    *x1 = x + radius < width ? x + radius : width - 1u;
    *y1 = y + radius < height ? y + radius : height - 1u;
}

// does an event stamped t_q support one stamped t_i?  One subtraction and one comparison in f64; NaN: no.
ECAL_PA_HD bool nf_supports(double t_i, double t_q, double dt) { return (t_i - t_q) <= dt; }

// the position in [lo, hi) of the last entry of the ascending list sval that is < i, or NF_NONE (lo == hi: an empty list)
ECAL_PA_HD uint32_t nf_last_before(const uint32_t *sval, uint32_t lo, uint32_t hi, uint32_t i) {
    uint32_t a = lo, b = hi;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        if (sval[m] < i) a = m + 1u;
        else b = m;
    }
    return a > lo ? a - 1u : NF_NONE;
}

// The verdict of the event at sorted position pos (1 keep, 0 remove) from the index: skey / sval the sorted pairs, sts the stamps in
// sorted order, start [plane + 1].  *off_grid: the event has no pixel.  The walk ends as soon as min_support is reached.
ECAL_PA_HD uint8_t nf_position_verdict(uint32_t pos, const uint32_t *skey, const uint32_t *sval, const double *sts, const uint32_t *start,
                                       uint32_t width, uint32_t height, uint32_t radius, uint32_t min_support, uint32_t include_self, double dt,
                                       bool *off_grid) {
    const uint32_t key = skey[pos];
    *off_grid = key == width * height;
    if (*off_grid) return 1;
    const uint32_t i = sval[pos];
    const double t_i = sts[pos];
    uint32_t x0, x1, y0, y1;
    nf_window(key % width, key / width, radius, width, height, &x0, &x1, &y0, &y1);
    uint32_t support = 0;
    for (uint32_t qy = y0; qy <= y1 && support < min_support; qy++)
        for (uint32_t qx = x0; qx <= x1 && support < min_support; qx++) {
            const uint32_t q = qy * width + qx;
            uint32_t at;
            if (q == key) {
                if (!include_self) continue;
                at = pos > start[q] ? pos - 1u : NF_NONE;   // (the list ascends: the entry in front is the last one before i)
            } else {
                at = nf_last_before(sval, start[q], start[q + 1u], i);
            }
            if (at != NF_NONE && nf_supports(t_i, sts[at], dt)) support++;
        }
    return (uint8_t) (support >= min_support ? 1u : 0u);
}

// ---- host: the rule as it is stated -----------------------------------------------------------------------------------------------------
// verdict [n]: 1 keep, 0 remove.  The options must have passed nf_options_error.
inline FilterTotals nf_verdict_sequential(const uint8_t *rec, uint64_t n, const NoiseOptions &o, uint8_t *verdict) {
    FilterTotals t{n, 0, 0, 0};
    const size_t plane = (size_t) o.width * o.height;
    std::vector<double> last(plane, 0.0);
    std::vector<uint8_t> seen(plane, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *r = rec + i * PA_RECORD_BYTES;
        const uint32_t p = ecal_activity::pa_record_pixel(r, o.width, o.height);
        if (p == PA_OFF_GRID) {
            verdict[i] = 1;
            t.n_off_grid++;
            t.n_kept++;
            continue;
        }
        const double t_i = ecal_activity::pa_load_f64(r);
        uint32_t x0, x1, y0, y1;
        nf_window(p % o.width, p / o.width, o.radius, o.width, o.height, &x0, &x1, &y0, &y1);
        uint32_t support = 0;
        for (uint32_t qy = y0; qy <= y1; qy++)
            for (uint32_t qx = x0; qx <= x1; qx++) {
                const uint32_t q = qy * o.width + qx;
                if (q == p && !o.include_self) continue;
                if (seen[q] && nf_supports(t_i, last[q], o.dt)) support++;
            }
        verdict[i] = (uint8_t) (support >= o.min_support ? 1u : 0u);
        if (verdict[i]) t.n_kept++;
        else t.n_removed++;
        last[p] = t_i;
        seen[p] = 1;
    }
    return t;
}

// ---- host: the kernels' scheme ------------------------------------------------------------------------------------------------------------
// keys, a stable sort, the start table, the gathered stamps, every sorted position on its own (here: backwards).  n < 2^32.
inline FilterTotals nf_verdict_indexed(const uint8_t *rec, uint64_t n, const NoiseOptions &o, uint8_t *verdict) {
    FilterTotals t{n, 0, 0, 0};
    const uint32_t plane = o.width * o.height, cnt = (uint32_t) n;
    std::vector<uint32_t> key(cnt), sval(cnt), skey(cnt), start((size_t) plane + 1);
    std::vector<double> sts(cnt);
    for (uint32_t i = 0; i < cnt; i++) key[i] = nf_record_key(rec + (size_t) i * PA_RECORD_BYTES, o.width, o.height);
    std::iota(sval.begin(), sval.end(), 0u);
    const uint32_t mask = (uint32_t) ((1ull << nf_key_bits(plane)) - 1ull);   // (the sort looks at these bits alone: they hold every key)
    std::stable_sort(sval.begin(), sval.end(), [&](uint32_t a, uint32_t b) { return (key[a] & mask) < (key[b] & mask); });
    for (uint32_t pos = 0; pos < cnt; pos++) {
        skey[pos] = key[sval[pos]];
        sts[pos] = ecal_activity::pa_load_f64(rec + (size_t) sval[pos] * PA_RECORD_BYTES);
    }
    for (uint32_t p = 0; p <= plane; p++) start[p] = (uint32_t) (std::lower_bound(skey.begin(), skey.end(), p) - skey.begin());
    for (uint32_t pos = cnt; pos-- > 0;) {
        bool og;
        const uint8_t v = nf_position_verdict(pos, skey.data(), sval.data(), sts.data(), start.data(), o.width, o.height, o.radius, o.min_support,
                                              o.include_self, o.dt, &og);
        verdict[sval[pos]] = v;
        t.n_off_grid += og ? 1u : 0u;
        if (v) t.n_kept++;
        else t.n_removed++;
    }
    return t;
}

// ---- host: the compaction by a verdict array (pa_filter_sequential's, with the verdicts given) ---------------------------------------------
// out: room for n records, not overlapping rec.  Returns the kept records' count.
inline uint64_t nf_compact(const uint8_t *rec, uint64_t n, const uint8_t *verdict, uint8_t *out) {
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n; i++)
        if (verdict[i]) memcpy(out + (kept++) * PA_RECORD_BYTES, rec + i * PA_RECORD_BYTES, PA_RECORD_BYTES);
    return kept;
}
}  // namespace ecal_noise
