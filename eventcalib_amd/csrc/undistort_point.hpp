// Undistortion of a pixel with the solved camera — one restatement of include/ecal.h, "undistortion", for the kernels
// (ecal_undistort.hip), the host entry point (ecal_undistort_points_host) and the CPU test (tests/cpp/check_undistort.cpp).
//
// The solver's intrinsics are the INVERSE model: pixel -> ideal ray is a closed-form polynomial (spline_residual.hpp, residual_ray), so a
// point is ~25 f64 operations and nothing is iterated.  Every operation below is one IEEE f64 operation rounded on its own: the
// translation units that include this header are built with -ffp-contract=off, a division is a division, and the rounding to a canvas
// pixel is spelled out (ud_round_half_away) instead of left to a library.  Only tan (FISHEYE) is not correctly rounded.
// design/20_undistort.md has the reasoning.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_UD_HD __host__ __device__ __forceinline__
#else
#define ECAL_UD_HD inline
#endif

namespace ecal_undistort {

enum : int { UD_RADIAL = 0, UD_FISHEYE = 1 };        // ECAL_CAMERA_RADIAL / ECAL_CAMERA_FISHEYE
enum : uint32_t { UD_SUBPIXEL = 0, UD_PIXEL = 1 };   // ECAL_UNDISTORT_SUBPIXEL / ECAL_UNDISTORT_PIXEL
enum : uint32_t { UD_KEPT = 0, UD_INVALID = 1, UD_OUTSIDE = 2 };

constexpr uint32_t UD_RECORD_BYTES = 25;    // f64 t, f64 x, f64 y, u8 polarity (little endian, packed)
constexpr uint32_t UD_MAX_CANVAS = 8192;    // out_width, out_height: 1 .. 8192
constexpr double UD_HALF_PI = 1.5707963267948966;
constexpr double UD_SMALL_R2 = 1e-16;

struct Camera {   // ecal_undistort_camera
    int model, reserved;
    double intr[9];    // fx fy cx cy k1..k5
    double out_k[4];   // fx' fy' cx' cy'
};
struct Options {   // ecal_undistort_options
    uint32_t mode, out_width, out_height, reserved;
    double off_x, off_y;
};
struct Totals {   // ecal_undistort_totals
    uint64_t n_events, n_invalid, n_outside, n_kept;
};
struct FrameTotals {   // ecal_undistort_frame_totals
    uint32_t n_pos, n_neg, n_invalid, n_outside;
};

ECAL_UD_HD double ud_load_f64(const uint8_t *p) {
    double v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

ECAL_UD_HD bool ud_finite(double v) { return v - v == 0.0; }   // (false on NaN and on +-inf)

// std::round: the nearest whole number, halves away from zero.  a - trunc(a) is exact.
ECAL_UD_HD double ud_round_half_away(double a) {
    const double t = trunc(a);
    const double d = a - t;
    if (fabs(d) >= 0.5) return t + (a < 0.0 ? -1.0 : 1.0);
    return t;
}

// (u, v) -> (u', v') of the ideal pinhole camera out_k; false: invalid (nothing is written)
ECAL_UD_HD bool ud_point(const Camera &c, double u, double v, double *up, double *vp) {
    const double fx = c.intr[0], fy = c.intr[1], cx = c.intr[2], cy = c.intr[3];
    const double k1 = c.intr[4], k2 = c.intr[5], k3 = c.intr[6], k4 = c.intr[7], k5 = c.intr[8];
    const double x = (u - cx) / fx, y = (v - cy) / fy;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2, r10 = r8 * r2;
    const double poly = ((((1.0 + k1 * r2) + k2 * r4) + k3 * r6) + k4 * r8) + k5 * r10;
    double s;
    bool ok;
    if (c.model == UD_FISHEYE && r2 > UD_SMALL_R2) {
        const double r = sqrt(r2);
        const double th = r * poly;
        ok = th >= 0.0 && th < UD_HALF_PI;
        s = ok ? tan(th) / r : 0.0;
    } else {
        s = poly;
        ok = poly > 0.0;
    }
    if (!ok) return false;
    const double xu = x * s, yu = y * s;
    const double uo = c.out_k[0] * xu + c.out_k[2], vo = c.out_k[1] * yu + c.out_k[3];
    if (!ud_finite(uo) || !ud_finite(vo)) return false;
    *up = uo;
    *vp = vo;
    return true;
}

// What becomes of an event at (u, v): UD_KEPT with the record's new coordinates in (*ox, *oy) — u', v' (SUBPIXEL) or the canvas
// pixel X, Y as f64 (PIXEL) —, UD_INVALID, or UD_OUTSIDE (PIXEL: the pixel is not on the canvas)
ECAL_UD_HD uint32_t ud_event(const Camera &c, const Options &o, double u, double v, double *ox, double *oy) {
    double up, vp;
    if (!ud_point(c, u, v, &up, &vp)) return UD_INVALID;
    if (o.mode == UD_PIXEL) {
        const double X = ud_round_half_away(up + o.off_x), Y = ud_round_half_away(vp + o.off_y);
        if (!(X >= 0.0 && X < (double) o.out_width && Y >= 0.0 && Y < (double) o.out_height)) return UD_OUTSIDE;
        up = X;
        vp = Y;
    }
    *ox = up;
    *oy = vp;
    return UD_KEPT;
}

// ---- host: checks ------------------------------------------------------------------------------------------------------------------------
// null: fine; else the field that is refused
inline const char *ud_camera_error(const Camera &c) {
    static const char *const k_names[5] = {"k1 must be finite", "k2 must be finite", "k3 must be finite", "k4 must be finite", "k5 must be finite"};
    if (c.model != UD_RADIAL && c.model != UD_FISHEYE) return "model must be ECAL_CAMERA_RADIAL or ECAL_CAMERA_FISHEYE";
    if (c.reserved != 0) return "reserved must be 0";
    if (!(ud_finite(c.intr[0]) && c.intr[0] > 0.0)) return "fx must be finite and above 0";
    if (!(ud_finite(c.intr[1]) && c.intr[1] > 0.0)) return "fy must be finite and above 0";
    for (int i = 0; i < 5; i++)
        if (!ud_finite(c.intr[4 + i])) return k_names[i];
    if (!(ud_finite(c.out_k[0]) && c.out_k[0] > 0.0)) return "out_k fx' must be finite and above 0";
    if (!(ud_finite(c.out_k[1]) && c.out_k[1] > 0.0)) return "out_k fy' must be finite and above 0";
    return nullptr;
}

inline const char *ud_options_error(const Options &o) {
    if (o.mode != UD_SUBPIXEL && o.mode != UD_PIXEL) return "mode must be ECAL_UNDISTORT_SUBPIXEL or ECAL_UNDISTORT_PIXEL";
    if (o.reserved != 0) return "options reserved must be 0";
    if (o.mode == UD_PIXEL) {
        if (o.out_width < 1 || o.out_width > UD_MAX_CANVAS) return "out_width from 1 to 8192";
        if (o.out_height < 1 || o.out_height > UD_MAX_CANVAS) return "out_height from 1 to 8192";
        if (!ud_finite(o.off_x)) return "off_x must be finite";
        if (!ud_finite(o.off_y)) return "off_y must be finite";
    }
    return nullptr;
}

// EventFrame.cpp:39,48-49: the canvas is round(1.2 * size), the offset size * 0.1, as f64 products
inline Options ud_reference_canvas(uint32_t width, uint32_t height) {
    Options o;
    o.mode = UD_PIXEL;
    o.out_width = (uint32_t) ud_round_half_away(1.2 * (double) width);
    o.out_height = (uint32_t) ud_round_half_away(1.2 * (double) height);
    o.reserved = 0;
    o.off_x = (double) width * 0.1;
    o.off_y = (double) height * 0.1;
    return o;
}

// ---- host: the stream form, one walk -------------------------------------------------------------------------------------------------------
// out: room for n records, not overlapping rec.  Kept records: the stamp and the polarity byte as they are, x and y replaced.
inline Totals ud_events_sequential(const Camera &c, const Options &o, const uint8_t *rec, uint64_t n, uint8_t *out) {
    Totals t{n, 0, 0, 0};
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *r = rec + i * UD_RECORD_BYTES;
        double ox, oy;
        const uint32_t what = ud_event(c, o, ud_load_f64(r + 8), ud_load_f64(r + 16), &ox, &oy);
        if (what == UD_INVALID) t.n_invalid++;
        else if (what == UD_OUTSIDE) t.n_outside++;
        else {
            uint8_t *d = out + t.n_kept * UD_RECORD_BYTES;
            memcpy(d, r, 8);
            memcpy(d + 8, &ox, 8);
            memcpy(d + 16, &oy, 8);
            d[24] = r[24];
            t.n_kept++;
        }
    }
    return t;
}
}  // namespace ecal_undistort
