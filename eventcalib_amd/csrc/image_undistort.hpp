// Image undistortion with the solved camera — one restatement of include/ecal.h, "image undistortion", for the kernels
// (ecal_image.hip), the host entry points (ecal_undistort_image_host, ecal_distort_points_host, ecal_camera_monotone_radius) and the
// CPU test (tests/cpp/check_image_undistort.cpp).  design/22_image_undistort.md has the reasoning.
//
// Two methods.  REFERENCE is PinholeCamera::undistortImage (core/sensor/src/PinholeCamera.cpp:128-214) — every source pixel is
// carried to the canvas with ud_point, a canvas pixel is the inverse-squared-distance average of the carried pixels within 2 px —
// with an order of accumulation of this project's own (the reference's is its kd-tree's traversal); OpenCV's float paths are not
// reproduced bit for bit: parity unpinned.  BILINEAR goes the other way: the forward projection (ideal pixel -> sensor pixel, eight
// Newton steps on the solved inverse model) gives cv::initUndistortRectifyMap's maps, and a canvas pixel is the bilinear sample of
// the source there.
//
// Every operation below is one IEEE f64 or f32 operation rounded on its own: the translation units that include this header are built
// with -ffp-contract=off.  tan (ud_point, FISHEYE) and atan (img_distort_point, FISHEYE) are the only operations that are not
// correctly rounded.
#pragma once
#include "undistort_point.hpp"

#include <vector>

namespace ecal_image {

using ecal_undistort::Camera;
using ecal_undistort::ud_finite;
using ecal_undistort::ud_point;
using ecal_undistort::ud_round_half_away;
using ecal_undistort::UD_FISHEYE;

enum : uint32_t { IMG_REFERENCE = 0, IMG_BILINEAR = 1 };             // ECAL_IMAGE_REFERENCE / ECAL_IMAGE_BILINEAR
enum : uint8_t { IMG_DISTORT_INVALID = 1, IMG_DISTORT_NOT_CONVERGED = 2 };   // ECAL_DISTORT_INVALID / ECAL_DISTORT_NOT_CONVERGED

constexpr uint32_t IMG_MAX_SIDE = 8192;            // sensor and canvas: 1 .. 8192 a side
constexpr double IMG_RADIUS2 = 4.0;                // a neighbour: d2 < 4.0 (strict)
constexpr double IMG_DBL_EPSILON = 2.220446049250313e-16;
constexpr double IMG_MIN_D2 = 100.0 * IMG_DBL_EPSILON;   // (exact in f64)
constexpr uint32_t IMG_PAD = 2;                    // cells around the canvas: floor(cu) from -2 to out_width + 1
constexpr uint32_t IMG_MAX_PER_SOURCE = 13;        // whole-number points inside an open disc of radius 2, at most
constexpr uint32_t IMG_NEWTON_STEPS = 8;
constexpr uint32_t IMG_MONOTONE_SAMPLES = 4096;
constexpr double IMG_CONVERGED_PX = 1e-9;
constexpr uint32_t IMG_NO_CELL = 0xFFFFFFFFu;

struct Options {   // ecal_image_options
    uint32_t method, channels, out_width, out_height, normalize, reserved;
    double off_x, off_y;
};
struct Info {   // ecal_image_info
    Options opt;
    uint32_t width, height;
    uint64_t n_invalid_sources, n_empty, n_entries;
    uint32_t max_neighbours, truncated;
    uint64_t bytes;
    double r_lim;
    uint64_t n_invalid, n_not_converged;
};
// what the forward projection needs beside the camera: once per camera and sensor, on the host (img_forward)
struct Forward {
    double r_lim, g_lim, r0_scale, px_scale;   // g(r_lim); r_lim / g(r_lim); max(fx, fy)
    uint32_t truncated, reserved;
};

// ---- the forward projection -------------------------------------------------------------------------------------------------------------
// poly(s) as ud_point spells it, s = r*r
ECAL_UD_HD double img_poly(const Camera &c, double s) {
    const double k1 = c.intr[4], k2 = c.intr[5], k3 = c.intr[6], k4 = c.intr[7], k5 = c.intr[8];
    const double s2 = s * s, s3 = s2 * s, s4 = s3 * s, s5 = s4 * s;
    return ((((1.0 + k1 * s) + k2 * s2) + k3 * s3) + k4 * s4) + k5 * s5;
}
// dp(s) = k1 + 2 k2 s + 3 k3 s^2 + 4 k4 s^3 + 5 k5 s^4, summed left to right, each coefficient (n * kn) first
ECAL_UD_HD double img_dpoly(const Camera &c, double s) {
    const double k1 = c.intr[4], k2 = c.intr[5], k3 = c.intr[6], k4 = c.intr[7], k5 = c.intr[8];
    const double s2 = s * s, s3 = s2 * s, s4 = s3 * s;
    return (((k1 + (2.0 * k2) * s) + (3.0 * k3) * s2) + (4.0 * k4) * s3) + (5.0 * k5) * s4;
}
// g(r) = r * poly(r*r): the distorted radius (RADIAL) or angle (FISHEYE) of the normalised sensor radius r
ECAL_UD_HD double img_g(const Camera &c, double r) { return r * img_poly(c, r * r); }
// g'(r) = poly(s) + (2 s) * dp(s)
ECAL_UD_HD double img_dg(const Camera &c, double r) {
    const double s = r * r;
    return img_poly(c, s) + (2.0 * s) * img_dpoly(c, s);
}

// (u', v') of the ideal camera out_k -> (u, v) of the sensor.  Returns the flag byte: 0, IMG_DISTORT_INVALID (nothing is written) or
// IMG_DISTORT_NOT_CONVERGED (the point is written all the same).  No branch depends on the data but the two selects below.
ECAL_UD_HD uint8_t img_distort_point(const Camera &c, const Forward &f, double up, double vp, double *u, double *v) {
    const double fx = c.intr[0], fy = c.intr[1], cx = c.intr[2], cy = c.intr[3];
    const double xu = (up - c.out_k[2]) / c.out_k[0], yu = (vp - c.out_k[3]) / c.out_k[1];
    const double rho2 = xu * xu + yu * yu;
    const bool small = rho2 <= ecal_undistort::UD_SMALL_R2;
    const double rho = sqrt(rho2);
    const double T = c.model == UD_FISHEYE ? atan(rho) : rho;
    const bool inside = small || T <= f.g_lim;   // (false on a NaN)
    double r = T * f.r0_scale;
    for (uint32_t k = 0; k < IMG_NEWTON_STEPS; k++) {   // (a fixed count: no early exit)
        const double e = img_g(c, r) - T;
        r = r - e / img_dg(c, r);
        r = r < 0.0 ? 0.0 : r;
        r = r > f.r_lim ? f.r_lim : r;
    }
    const double res = fabs(img_g(c, r) - T) * f.px_scale;
    const double scale = small ? 1.0 : r / rho;
    const double uo = fx * (xu * scale) + cx, vo = fy * (yu * scale) + cy;
    if (!inside || !ud_finite(uo) || !ud_finite(vo)) return IMG_DISTORT_INVALID;
    *u = uo;
    *v = vo;
    return (!small && res > IMG_CONVERGED_PX) ? IMG_DISTORT_NOT_CONVERGED : (uint8_t) 0;
}

// One canvas pixel of the BILINEAR maps: (X, Y) -> map_x, map_y (f32; -1 where invalid), the valid byte; returns the flag byte
ECAL_UD_HD uint8_t img_map_pixel(const Camera &c, const Forward &f, const Options &o, uint32_t X, uint32_t Y, float *mx, float *my, uint8_t *valid) {
    double u = 0.0, v = 0.0;
    const uint8_t flag = img_distort_point(c, f, (double) X - o.off_x, (double) Y - o.off_y, &u, &v);
    const bool ok = flag != IMG_DISTORT_INVALID;
    *mx = ok ? (float) u : -1.0f;
    *my = ok ? (float) v : -1.0f;
    *valid = ok ? 1 : 0;
    return flag;
}

// the bilinear sample of channel ch of one frame at (mx, my): f32, each operation rounded on its own; a tap off the sensor is 0
ECAL_UD_HD float img_bilinear(const uint8_t *src, uint32_t W, uint32_t H, uint32_t C, uint32_t ch, float mx, float my) {
    if (!(mx > -1.0f && mx < (float) W && my > -1.0f && my < (float) H)) return 0.0f;   // (no tap on the sensor; a NaN too)
    const float x0 = floorf(mx), y0 = floorf(my);
    const float ax = mx - x0, ay = my - y0;
    const int32_t ix = (int32_t) x0, iy = (int32_t) y0;   // -1 .. W - 1, -1 .. H - 1
    const bool l = ix >= 0, r = ix + 1 < (int32_t) W, t = iy >= 0, b = iy + 1 < (int32_t) H;
    const size_t row0 = (size_t) (t ? iy : 0) * W, row1 = (size_t) (b ? iy + 1 : 0) * W;
    const size_t c0 = (size_t) (l ? ix : 0), c1 = (size_t) (r ? ix + 1 : 0);
    const float s00 = t && l ? (float) src[(row0 + c0) * C + ch] : 0.0f, s01 = t && r ? (float) src[(row0 + c1) * C + ch] : 0.0f;
    const float s10 = b && l ? (float) src[(row1 + c0) * C + ch] : 0.0f, s11 = b && r ? (float) src[(row1 + c1) * C + ch] : 0.0f;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float top = s00 * bx + s01 * ax, bot = s10 * bx + s11 * ax;
    return top * by + bot * ay;
}

// ---- REFERENCE: positions, neighbours, weights ------------------------------------------------------------------------------------------
// source pixel (col, row) -> its canvas position (cu, cv) and cell key (floor(cv) + 2) * (out_width + 4) + floor(cu) + 2; IMG_NO_CELL:
// more than 2 px off the canvas (it neighbours nothing) or invalid (*invalid set)
ECAL_UD_HD uint32_t img_source_cell(const Camera &c, const Options &o, uint32_t col, uint32_t row, double *cu, double *cv, bool *invalid) {
    double up = 0.0, vp = 0.0;
    const bool ok = ud_point(c, (double) col, (double) row, &up, &vp);
    *invalid = !ok;
    *cu = 0.0;
    *cv = 0.0;
    if (!ok) return IMG_NO_CELL;
    const double x = up + o.off_x, y = vp + o.off_y;
    const double fx = floor(x), fy = floor(y);
    if (!(fx >= -2.0 && fx <= (double) o.out_width + 1.0 && fy >= -2.0 && fy <= (double) o.out_height + 1.0)) return IMG_NO_CELL;
    *cu = x;
    *cv = y;
    return (uint32_t) ((int32_t) fy + 2) * (o.out_width + 2u * IMG_PAD) + (uint32_t) ((int32_t) fx + 2);
}
ECAL_UD_HD uint32_t img_cell_count(const Options &o) { return (o.out_width + 2u * IMG_PAD) * (o.out_height + 2u * IMG_PAD); }   // <= 8196^2

// d2 of canvas pixel (j, i) and a source at (cu, cv); a neighbour iff d2 < 4.0
ECAL_UD_HD double img_d2(uint32_t j, uint32_t i, double cu, double cv) {
    const double dx = (double) j - cu, dy = (double) i - cv;
    return dx * dx + dy * dy;
}
ECAL_UD_HD double img_weight(double d2) { return 1.0 / (d2 > IMG_MIN_D2 ? d2 : IMG_MIN_D2); }

// The neighbours of canvas pixel (j, i) in the stated order — ascending (floor(cv), floor(cu), idx) —: the sources of the 4 x 4 cells
// floor(cu) = j - 2 .. j + 1, floor(cv) = i - 2 .. i + 1, a row of four cells being one run of the sorted sources (start: the first
// sorted position of every cell, n_cells + 1 words; sidx: the sources sorted by (cell, idx)).  emit(idx, w) per neighbour.
template <class Emit>
ECAL_UD_HD uint32_t img_neighbours(const Options &o, uint32_t j, uint32_t i, const uint32_t *start, const uint32_t *sidx, const double *cu,
                                   const double *cv, Emit emit) {
    const uint32_t cw = o.out_width + 2u * IMG_PAD;
    uint32_t n = 0;
    for (uint32_t cy = i; cy < i + 4u; cy++) {
        const uint32_t k0 = cy * cw + j;
        const uint32_t a = start[k0], b = start[k0 + 4u];
        for (uint32_t q = a; q < b; q++) {
            const uint32_t idx = sidx[q];
            const double d2 = img_d2(j, i, cu[idx], cv[idx]);
            if (d2 < IMG_RADIUS2) {
                emit(idx, img_weight(d2));
                n++;
            }
        }
    }
    return n;
}

// one channel's average from its accumulators (no neighbour: 0)
ECAL_UD_HD float img_average(float acc, double wsum, bool any) { return any ? (float) ((double) acc * (1.0 / wsum)) : 0.0f; }
// one more neighbour
ECAL_UD_HD float img_accumulate(float acc, double w, uint8_t v) { return acc + (float) (w * (double) v); }

// ---- both methods: f32 value -> u8 -------------------------------------------------------------------------------------------------------
ECAL_UD_HD double img_norm_scale(float mn, float mx) {
    const double span = (double) mx - (double) mn;
    return span > IMG_DBL_EPSILON ? 255.0 / span : 0.0;
}
ECAL_UD_HD uint8_t img_saturate(double r) { return (uint8_t) (r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r)); }   // (a NaN: 0)
// normalize 1: cv::normalize(NORM_MINMAX, 0 .. 255) of one frame; rint: ties to even
ECAL_UD_HD uint8_t img_to_u8_normalized(float val, float mn, double scale) { return img_saturate(rint((double) val * scale - (double) mn * scale)); }
// normalize 0
ECAL_UD_HD uint8_t img_to_u8(float val) { return img_saturate(ud_round_half_away((double) val)); }

// ---- host: checks, the reference canvas, the limit --------------------------------------------------------------------------------------
inline const char *img_options_error(const Options &o) {
    if (o.method != IMG_REFERENCE && o.method != IMG_BILINEAR) return "method must be ECAL_IMAGE_REFERENCE or ECAL_IMAGE_BILINEAR";
    if (o.channels != 1 && o.channels != 3) return "channels must be 1 or 3";
    if (o.out_width < 1 || o.out_width > IMG_MAX_SIDE) return "out_width from 1 to 8192";
    if (o.out_height < 1 || o.out_height > IMG_MAX_SIDE) return "out_height from 1 to 8192";
    if (o.normalize > 1) return "normalize must be 0 or 1";
    if (o.reserved != 0) return "options reserved must be 0";
    if (!ud_finite(o.off_x)) return "off_x must be finite";
    if (!ud_finite(o.off_y)) return "off_y must be finite";
    return nullptr;
}
inline const char *img_sensor_error(uint32_t width, uint32_t height) {
    if (width < 1 || width > IMG_MAX_SIDE) return "width from 1 to 8192";
    if (height < 1 || height > IMG_MAX_SIDE) return "height from 1 to 8192";
    return nullptr;
}

// PinholeCamera.cpp:132-135: the canvas is round(1.2 * size), the offset round(size * 0.1) — ROUNDED, unlike EventFrame's
inline Options img_reference_options(uint32_t width, uint32_t height) {
    Options o;
    o.method = IMG_REFERENCE;
    o.channels = 3;
    o.out_width = (uint32_t) ud_round_half_away(1.2 * (double) width);
    o.out_height = (uint32_t) ud_round_half_away(1.2 * (double) height);
    o.normalize = 1;
    o.reserved = 0;
    o.off_x = ud_round_half_away((double) width * 0.1);
    o.off_y = ud_round_half_away((double) height * 0.1);
    return o;
}

// r_lim: 1.05 x the largest normalised radius of the four outer corners (-0.5 | W - 0.5, -0.5 | H - 0.5), cut back to the last of 4096
// samples before g' stops being positive (truncated)
inline Forward img_forward(const Camera &c, uint32_t width, uint32_t height) {
    const double fx = c.intr[0], fy = c.intr[1], cx = c.intr[2], cy = c.intr[3];
    const double us[2] = {-0.5, (double) width - 0.5}, vs[2] = {-0.5, (double) height - 0.5};
    double rmax = 0.0;
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const double x = (us[a] - cx) / fx, y = (vs[b] - cy) / fy;
            const double r = sqrt(x * x + y * y);
            if (r > rmax) rmax = r;
        }
    const double r0 = 1.05 * rmax;
    Forward f;
    f.r_lim = r0;
    f.truncated = 0;
    f.reserved = 0;
    for (uint32_t m = 1; m <= IMG_MONOTONE_SAMPLES; m++) {
        const double r = (r0 * (double) m) / (double) IMG_MONOTONE_SAMPLES;
        if (!(img_dg(c, r) > 0.0)) {
            f.r_lim = (r0 * (double) (m - 1)) / (double) IMG_MONOTONE_SAMPLES;
            f.truncated = 1;
            break;
        }
    }
    f.g_lim = img_g(c, f.r_lim);
    f.r0_scale = f.r_lim / f.g_lim;
    f.px_scale = fx > fy ? fx : fy;
    return f;
}

// ---- host: one sequential walk per method ------------------------------------------------------------------------------------------------
// The REFERENCE tables of a camera, sensor and canvas: off [canvas pixels + 1], idx / w [n_entries] in the stated order
struct Table {
    std::vector<uint32_t> off, idx;
    std::vector<double> w;
    uint64_t n_invalid_sources = 0, n_empty = 0;
    uint32_t max_neighbours = 0;
};
inline Table img_table_sequential(const Camera &c, uint32_t W, uint32_t H, const Options &o) {
    Table t;
    const size_t n_src = (size_t) W * H, n_cells = img_cell_count(o), np = (size_t) o.out_width * o.out_height;
    std::vector<double> cu(n_src), cv(n_src);
    std::vector<uint32_t> key(n_src), start(n_cells + 2, 0), sidx;
    for (uint32_t row = 0; row < H; row++)
        for (uint32_t col = 0; col < W; col++) {
            const size_t idx = (size_t) row * W + col;
            bool inv;
            key[idx] = img_source_cell(c, o, col, row, &cu[idx], &cv[idx], &inv);
            t.n_invalid_sources += inv ? 1 : 0;
            if (key[idx] != IMG_NO_CELL) start[key[idx] + 1]++;
        }
    for (size_t k = 0; k < n_cells; k++) start[k + 1] += start[k];   // start[k]: the first sorted position of cell k
    sidx.resize(start[n_cells]);
    {
        std::vector<uint32_t> at(start.begin(), start.begin() + n_cells);
        for (size_t idx = 0; idx < n_src; idx++)   // (ascending idx inside every cell)
            if (key[idx] != IMG_NO_CELL) sidx[at[key[idx]]++] = (uint32_t) idx;
    }
    t.off.assign(np + 1, 0);
    for (uint32_t i = 0; i < o.out_height; i++)
        for (uint32_t j = 0; j < o.out_width; j++) {
            const size_t p = (size_t) i * o.out_width + j;
            const uint32_t n = img_neighbours(o, j, i, start.data(), sidx.data(), cu.data(), cv.data(), [&](uint32_t idx, double w) {
                t.idx.push_back(idx);
                t.w.push_back(w);
            });
            t.off[p + 1] = (uint32_t) t.idx.size();
            t.n_empty += n ? 0 : 1;
            if (n > t.max_neighbours) t.max_neighbours = n;
        }
    return t;
}

// The BILINEAR maps [out_height][out_width] and the counts behind them
struct Maps {
    std::vector<float> mx, my;
    std::vector<uint8_t> valid;
    uint64_t n_invalid = 0, n_not_converged = 0;
};
inline Maps img_maps_sequential(const Camera &c, const Forward &f, const Options &o) {
    Maps m;
    const size_t np = (size_t) o.out_width * o.out_height;
    m.mx.resize(np), m.my.resize(np), m.valid.resize(np);
    for (uint32_t Y = 0; Y < o.out_height; Y++)
        for (uint32_t X = 0; X < o.out_width; X++) {
            const size_t p = (size_t) Y * o.out_width + X;
            const uint8_t flag = img_map_pixel(c, f, o, X, Y, &m.mx[p], &m.my[p], &m.valid[p]);
            m.n_invalid += flag == IMG_DISTORT_INVALID ? 1 : 0;
            m.n_not_converged += flag == IMG_DISTORT_NOT_CONVERGED ? 1 : 0;
        }
    return m;
}

// the f32 values of one frame [out_height][out_width][C] -> u8, by the options' normalize; minmax (may be null): the frame's min, max
inline void img_finish_sequential(const Options &o, const float *val, uint8_t *dst, float *minmax) {
    const size_t n = (size_t) o.out_width * o.out_height * o.channels;
    float mn = val[0], mx = val[0];
    for (size_t k = 1; k < n; k++) {
        mn = val[k] < mn ? val[k] : mn;
        mx = val[k] > mx ? val[k] : mx;
    }
    if (minmax) minmax[0] = mn, minmax[1] = mx;
    const double scale = img_norm_scale(mn, mx);
    for (size_t k = 0; k < n; k++) dst[k] = o.normalize ? img_to_u8_normalized(val[k], mn, scale) : img_to_u8(val[k]);
}

// src [H][W][C] -> dst [out_height][out_width][C]; info (may be null) filled like a plan's, bytes 0
inline void img_undistort_sequential(const Camera &c, uint32_t W, uint32_t H, const Options &o, const uint8_t *src, uint8_t *dst, float *minmax,
                                     Info *info) {
    const uint32_t C = o.channels;
    const size_t np = (size_t) o.out_width * o.out_height;
    std::vector<float> val(np * C, 0.0f);
    Info I;
    memset(&I, 0, sizeof(I));
    I.opt = o;
    I.width = W;
    I.height = H;
    if (o.method == IMG_REFERENCE) {
        const Table t = img_table_sequential(c, W, H, o);
        for (size_t p = 0; p < np; p++) {
            float acc[3] = {0.0f, 0.0f, 0.0f};
            double wsum = 0.0;
            for (uint32_t e = t.off[p]; e < t.off[p + 1]; e++) {
                const uint8_t *s = src + (size_t) t.idx[e] * C;
                for (uint32_t ch = 0; ch < C; ch++) acc[ch] = img_accumulate(acc[ch], t.w[e], s[ch]);
                wsum = wsum + t.w[e];
            }
            for (uint32_t ch = 0; ch < C; ch++) val[p * C + ch] = img_average(acc[ch], wsum, t.off[p + 1] > t.off[p]);
        }
        I.n_invalid_sources = t.n_invalid_sources;
        I.n_empty = t.n_empty;
        I.n_entries = t.idx.size();
        I.max_neighbours = t.max_neighbours;
    } else {
        const Forward f = img_forward(c, W, H);
        const Maps m = img_maps_sequential(c, f, o);
        for (size_t p = 0; p < np; p++)
            for (uint32_t ch = 0; ch < C; ch++) val[p * C + ch] = img_bilinear(src, W, H, C, ch, m.mx[p], m.my[p]);
        I.r_lim = f.r_lim;
        I.truncated = f.truncated;
        I.n_invalid = m.n_invalid;
        I.n_not_converged = m.n_not_converged;
        I.n_empty = m.n_invalid;
    }
    img_finish_sequential(o, val.data(), dst, minmax);
    if (info) *info = I;
}
}  // namespace ecal_image
