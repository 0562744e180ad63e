"""The image undistortion rules of include/ecal.h ("image undistortion") in numpy, beside undistort_oracle.py: every line is one IEEE
f64 or f32 operation on arrays (plain * + - /, no **, nothing numpy could fuse), so RADIAL results are comparable bit for bit with the
library's; tan and atan (FISHEYE) are the operations that are not correctly rounded anywhere."""
import numpy as np

import undistort_oracle as UO

REFERENCE, BILINEAR = 0, 1
DISTORT_INVALID, DISTORT_NOT_CONVERGED = 1, 2
DBL_EPSILON = float(np.finfo(np.float64).eps)
MIN_D2 = 100.0 * DBL_EPSILON
F32 = np.float32

# ---- the cameras of the tests: name -> (model, intr, sensors) ----
K_BARREL = (-0.21, 0.07, -0.012, 0.0011, -0.00004)
CAMERAS = {
    "B346": (UO.RADIAL, (251.3, 249.8, 171.2, 129.9) + K_BARREL, (346, 260)),
    "B64": (UO.RADIAL, (48.0, 47.5, 31.2, 23.9) + K_BARREL, (64, 48)),
    "B37": (UO.RADIAL, (30.0, 29.0, 17.7, 14.1) + K_BARREL, (37, 29)),
    "P64": (UO.RADIAL, (48.0, 47.5, 31.2, 23.9, 0.15, 0.02, 0.0, 0.0, 0.0), (64, 48)),
    "F64": (UO.FISHEYE, (34.0, 34.0, 31.5, 23.5, -0.02, 0.003, 0.0, 0.0, 0.0), (64, 48)),
    "I40": (UO.RADIAL, (40.0, 41.0, 19.5, 14.25, 0.0, 0.0, 0.0, 0.0, 0.0), (40, 30)),
}


def camera(name):
    model, intr, (w, h) = CAMERAS[name]
    return UO.camera(model, intr), w, h


def options(method=REFERENCE, channels=3, out_width=1, out_height=1, normalize=0, off_x=0.0, off_y=0.0):
    return {"method": int(method), "channels": int(channels), "out_width": int(out_width), "out_height": int(out_height),
            "normalize": int(normalize), "off_x": float(off_x), "off_y": float(off_y)}


def reference_options(width, height):
    """PinholeCamera.cpp:132-135: out = round(1.2 * size), off = round(size * 0.1), 3 channels, normalize 1, REFERENCE"""
    r = UO.round_half_away
    return options(REFERENCE, 3, int(r(np.float64(1.2) * np.float64(width))), int(r(np.float64(1.2) * np.float64(height))), 1,
                   float(r(np.float64(width) * np.float64(0.1))), float(r(np.float64(height) * np.float64(0.1))))


# ---- REFERENCE ----
def table(cam, W, H, opt):
    """-> dict(off [np + 1] uint32, idx [n] uint32, w [n] float64, d2 [n], n_invalid_sources, n_empty, max_neighbours): every canvas
    pixel's neighbours in the order ascending (floor(cv), floor(cu), idx)"""
    ow, oh = opt["out_width"], opt["out_height"]
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    out, flag = UO.points(cam, np.stack([cols.ravel(), rows.ravel()], axis=1))
    cu = out[:, 0] + np.float64(opt["off_x"])
    cv = out[:, 1] + np.float64(opt["off_y"])
    fx, fy = np.floor(cu), np.floor(cv)
    keep = (flag == 0) & (fx >= -2.0) & (fx <= ow + 1.0) & (fy >= -2.0) & (fy <= oh + 1.0)
    src = np.nonzero(keep)[0]
    e_p, e_idx, e_d2, e_fy, e_fx = [], [], [], [], []
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            j = fx[src] + dx
            i = fy[src] + dy
            ddx = j - cu[src]
            ddy = i - cv[src]
            a = ddx * ddx
            b = ddy * ddy
            d2 = a + b
            ok = (d2 < 4.0) & (j >= 0) & (j < ow) & (i >= 0) & (i < oh)
            e_p.append((i[ok] * ow + j[ok]).astype(np.int64))
            e_idx.append(src[ok])
            e_d2.append(d2[ok])
            e_fy.append(fy[src][ok])
            e_fx.append(fx[src][ok])
    e_p, e_idx, e_d2, e_fy, e_fx = [np.concatenate(v) for v in (e_p, e_idx, e_d2, e_fy, e_fx)]
    order = np.lexsort((e_idx, e_fx, e_fy, e_p))
    e_p, e_idx, e_d2 = e_p[order], e_idx[order], e_d2[order]
    counts = np.bincount(e_p, minlength=ow * oh)
    off = np.zeros(ow * oh + 1, np.int64)
    off[1:] = np.cumsum(counts)
    w = 1.0 / np.maximum(e_d2, MIN_D2)
    return {"off": off.astype(np.uint32), "idx": e_idx.astype(np.uint32), "w": w, "d2": e_d2, "p": e_p,
            "n_invalid_sources": int((flag != 0).sum()), "n_empty": int((counts == 0).sum()), "max_neighbours": int(counts.max(initial=0)),
            "all_d2": _all_d2(cu, cv, keep, ow, oh)}


def _all_d2(cu, cv, keep, ow, oh):
    """d2 of every (source, canvas pixel) pair of the 4 x 4 candidates, on or off the canvas: the margin |d2 - 4| is taken over these"""
    fx, fy = np.floor(cu[keep]), np.floor(cv[keep])
    out = []
    for dy in range(-2, 4):
        for dx in range(-2, 4):
            ddx = (fx + dx) - cu[keep]
            ddy = (fy + dy) - cv[keep]
            out.append(ddx * ddx + ddy * ddy)
    return np.concatenate(out)


def reference_values(tab, frame, opt):
    """frame [H, W, C] uint8 -> the averages [oh, ow, C] float32"""
    C = opt["channels"]
    npix = opt["out_width"] * opt["out_height"]
    px = np.ascontiguousarray(frame, np.uint8).reshape(-1, C)
    off = tab["off"].astype(np.int64)
    rank = np.arange(tab["idx"].size, dtype=np.int64) - off[tab["p"]]
    acc = np.zeros((npix, C), F32)
    wsum = np.zeros(npix, np.float64)
    for r in range(tab["max_neighbours"]):
        sel = np.nonzero(rank == r)[0]
        p, w = tab["p"][sel], tab["w"][sel]
        term = (w[:, None] * px[tab["idx"][sel]].astype(np.float64)).astype(F32)
        acc[p] = acc[p] + term
        wsum[p] = wsum[p] + w
    some = wsum > 0.0
    inv = np.zeros(npix, np.float64)
    inv[some] = 1.0 / wsum[some]
    avg = (acc.astype(np.float64) * inv[:, None]).astype(F32)
    avg[~some] = 0.0
    return avg.reshape(opt["out_height"], opt["out_width"], C)


def to_u8(val, normalize):
    """one frame's f32 values -> (uint8, (min, max))"""
    val = np.asarray(val, F32)
    mn, mx = val.min(), val.max()
    if normalize:
        span = np.float64(mx) - np.float64(mn)
        scale = np.float64(255.0) / span if span > DBL_EPSILON else np.float64(0.0)
        a = val.astype(np.float64) * scale
        b = np.float64(mn) * scale
        r = np.rint(a - b)
    else:
        r = UO.round_half_away(val.astype(np.float64))
    return np.clip(r, 0.0, 255.0).astype(np.uint8), (F32(mn), F32(mx))


# ---- the forward projection ----
def _coeffs(cam):
    return [np.float64(v) for v in cam["intr"][4:]]


def poly(cam, s):
    k1, k2, k3, k4, k5 = _coeffs(cam)
    s2 = s * s
    s3 = s2 * s
    s4 = s3 * s
    s5 = s4 * s
    p = 1.0 + k1 * s
    p = p + k2 * s2
    p = p + k3 * s3
    p = p + k4 * s4
    p = p + k5 * s5
    return p


def dpoly(cam, s):
    k1, k2, k3, k4, k5 = _coeffs(cam)
    s2 = s * s
    s3 = s2 * s
    s4 = s3 * s
    d = k1 + (2.0 * k2) * s
    d = d + (3.0 * k3) * s2
    d = d + (4.0 * k4) * s3
    d = d + (5.0 * k5) * s4
    return d


def g(cam, r):
    return r * poly(cam, r * r)


def dg(cam, r):
    s = r * r
    t = (2.0 * s) * dpoly(cam, s)
    return poly(cam, s) + t


def monotone_radius(cam, W, H):
    """-> (r_lim, truncated)"""
    fx, fy, cx, cy = [np.float64(v) for v in cam["intr"][:4]]
    rmax = np.float64(0.0)
    for u in (np.float64(-0.5), np.float64(W) - 0.5):
        for v in (np.float64(-0.5), np.float64(H) - 0.5):
            x = (u - cx) / fx
            y = (v - cy) / fy
            rmax = max(rmax, np.sqrt(x * x + y * y))
    r0 = np.float64(1.05) * rmax
    m = np.arange(1, 4097, dtype=np.float64)
    with np.errstate(all="ignore"):
        bad = ~(dg(cam, (r0 * m) / 4096.0) > 0.0)
    if bad.any():
        first = int(np.nonzero(bad)[0][0]) + 1
        return float((r0 * np.float64(first - 1)) / 4096.0), 1
    return float(r0), 0


def distort_points(cam, W, H, uv):
    """uv [n, 2] of the ideal camera -> (out [n, 2] with 0, 0 where invalid, flag [n] uint8)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = [np.float64(v) for v in cam["intr"][:4]]
    fxo, fyo, cxo, cyo = [np.float64(v) for v in cam["out_k"]]
    r_lim, _ = monotone_radius(cam, W, H)
    r_lim = np.float64(r_lim)
    with np.errstate(all="ignore"):
        g_lim = g(cam, r_lim)
        r0_scale = r_lim / g_lim
        xu = (uv[:, 0] - cxo) / fxo
        yu = (uv[:, 1] - cyo) / fyo
        rho2 = xu * xu + yu * yu
        small = rho2 <= 1e-16
        rho = np.sqrt(rho2)
        T = np.arctan(rho) if cam["model"] == UO.FISHEYE else rho
        inside = small | (T <= g_lim)
        r = T * r0_scale
        for _ in range(8):
            e = g(cam, r) - T
            r = r - e / dg(cam, r)
            r = np.where(r < 0.0, 0.0, r)
            r = np.where(r > r_lim, r_lim, r)
        res = np.abs(g(cam, r) - T) * max(fx, fy)
        scale = np.where(small, 1.0, r / rho)
        u = fx * (xu * scale) + cx
        v = fy * (yu * scale) + cy
        valid = inside & np.isfinite(u) & np.isfinite(v)
        slow = valid & ~small & (res > 1e-9)
    out = np.zeros((uv.shape[0], 2), np.float64)
    out[valid, 0] = u[valid]
    out[valid, 1] = v[valid]
    flag = np.where(valid, np.where(slow, DISTORT_NOT_CONVERGED, 0), DISTORT_INVALID).astype(np.uint8)
    return out, flag


# ---- BILINEAR ----
def maps(cam, W, H, opt):
    """-> (map_x, map_y float32 [oh, ow], valid uint8 [oh, ow], flag uint8 [oh, ow])"""
    ow, oh = opt["out_width"], opt["out_height"]
    X, Y = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    out, flag = distort_points(cam, W, H, np.stack([X.ravel() - np.float64(opt["off_x"]), Y.ravel() - np.float64(opt["off_y"])], axis=1))
    ok = flag != DISTORT_INVALID
    mx = np.where(ok, out[:, 0].astype(F32), F32(-1.0)).astype(F32)
    my = np.where(ok, out[:, 1].astype(F32), F32(-1.0)).astype(F32)
    return mx.reshape(oh, ow), my.reshape(oh, ow), ok.astype(np.uint8).reshape(oh, ow), flag.reshape(oh, ow)


def bilinear_values(mx, my, frame):
    """frame [H, W, C] uint8 -> the samples [oh, ow, C] float32, every operation in f32"""
    frame = np.ascontiguousarray(frame, np.uint8)
    H, W, C = frame.shape
    mx, my = np.asarray(mx, F32), np.asarray(my, F32)
    with np.errstate(invalid="ignore"):
        any_tap = (mx > F32(-1.0)) & (mx < F32(W)) & (my > F32(-1.0)) & (my < F32(H))
    mxs, mys = np.where(any_tap, mx, F32(0.0)).astype(F32), np.where(any_tap, my, F32(0.0)).astype(F32)
    x0, y0 = np.floor(mxs), np.floor(mys)
    ax, ay = (mxs - x0).astype(F32), (mys - y0).astype(F32)
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    pad = np.zeros((H + 2, W + 2, C), F32)   # a tap off the sensor is 0
    pad[1:-1, 1:-1] = frame.astype(F32)
    s00, s01 = pad[iy + 1, ix + 1], pad[iy + 1, ix + 2]
    s10, s11 = pad[iy + 2, ix + 1], pad[iy + 2, ix + 2]
    ax, ay = ax[..., None], ay[..., None]
    bx, by = F32(1.0) - ax, F32(1.0) - ay
    top = s00 * bx + s01 * ax
    bot = s10 * bx + s11 * ax
    val = top * by + bot * ay
    assert val.dtype == F32
    val[~any_tap] = 0.0
    return val


# ---- one frame, either method ----
def undistort(cam, W, H, opt, frame, tab=None, mp=None):
    """frame [H, W, C] uint8 -> (picture [oh, ow, C] uint8, (min, max))"""
    frame = np.ascontiguousarray(frame, np.uint8).reshape(H, W, opt["channels"])
    if opt["method"] == REFERENCE:
        val = reference_values(tab if tab is not None else table(cam, W, H, opt), frame, opt)
    else:
        mx, my = (mp if mp is not None else maps(cam, W, H, opt))[:2]
        val = bilinear_values(mx, my, frame)
    return to_u8(val, opt["normalize"])
