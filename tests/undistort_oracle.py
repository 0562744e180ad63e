"""The undistortion rule of include/ecal.h ("undistortion") in numpy: every line is one IEEE f64 operation on arrays (plain * + - /,
no **, nothing numpy could fuse), so RADIAL results are comparable bit for bit with the library's; tan (FISHEYE) is the one operation
that is not correctly rounded anywhere."""
import numpy as np

RADIAL, FISHEYE = 0, 1
SUBPIXEL, PIXEL = 0, 1
HALF_PI = 1.5707963267948966
RECORD = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])   # packed: 25 bytes
assert RECORD.itemsize == 25


def camera(model, intr, out_k=None):
    intr = [float(v) for v in intr]
    assert len(intr) == 9
    return {"model": int(model), "intr": intr, "out_k": [float(v) for v in (intr[:4] if out_k is None else out_k)]}


def round_half_away(a):
    """std::round: trunc(a) + (|a - trunc(a)| >= 0.5) * sign(a); the subtraction is exact."""
    a = np.asarray(a, np.float64)
    t = np.trunc(a)
    step = np.where(a < 0.0, -1.0, 1.0)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(a - t) >= 0.5, t + step, t)


def reference_canvas(width, height):
    """EventFrame.cpp:39,48-49 -> (out_width, out_height, off_x, off_y)"""
    return (int(round_half_away(np.float64(1.2) * np.float64(width))), int(round_half_away(np.float64(1.2) * np.float64(height))),
            float(np.float64(width) * np.float64(0.1)), float(np.float64(height) * np.float64(0.1)))


def points(cam, uv):
    """uv [n, 2] -> (out [n, 2] with 0, 0 where invalid, flag [n] uint8: 1 invalid)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    fx, fy, cx, cy, k1, k2, k3, k4, k5 = [np.float64(v) for v in cam["intr"]]
    fxo, fyo, cxo, cyo = [np.float64(v) for v in cam["out_k"]]
    with np.errstate(all="ignore"):
        u, v = uv[:, 0], uv[:, 1]
        x = (u - cx) / fx
        y = (v - cy) / fy
        xx = x * x
        yy = y * y
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        r10 = r8 * r2
        a = k1 * r2
        poly = 1.0 + a
        a = k2 * r4
        poly = poly + a
        a = k3 * r6
        poly = poly + a
        a = k4 * r8
        poly = poly + a
        a = k5 * r10
        poly = poly + a
        c = poly.copy()
        valid = poly > 0.0
        if cam["model"] == FISHEYE:
            big = r2 > 1e-16
            r = np.sqrt(r2)
            th = r * poly
            tn = np.tan(th)
            cf = tn / r
            c = np.where(big, cf, c)
            valid = np.where(big, (th >= 0.0) & (th < HALF_PI), valid)
        xc = x * c
        yc = y * c
        up = fxo * xc
        up = up + cxo
        vp = fyo * yc
        vp = vp + cyo
        valid = valid & np.isfinite(up) & np.isfinite(vp)
    out = np.zeros((uv.shape[0], 2), np.float64)
    out[valid, 0] = up[valid]
    out[valid, 1] = vp[valid]
    return out, (~valid).astype(np.uint8)


def classify(cam, opt, uv):
    """-> (xy [n, 2]: what a kept record carries, what [n]: 0 kept, 1 invalid, 2 outside).  opt: dict(mode, out_width, out_height,
    off_x, off_y)."""
    out, flag = points(cam, uv)
    what = flag.astype(np.int64)
    if opt["mode"] == PIXEL:
        X = round_half_away(out[:, 0] + np.float64(opt["off_x"]))
        Y = round_half_away(out[:, 1] + np.float64(opt["off_y"]))
        inside = (X >= 0.0) & (X < float(opt["out_width"])) & (Y >= 0.0) & (Y < float(opt["out_height"]))
        what = np.where(flag != 0, 1, np.where(inside, 0, 2))
        out = np.stack([X, Y], axis=1)
    return out, what


def events(cam, opt, rec_bytes):
    """packed records (uint8 [n * 25]) -> (kept records as uint8 [n_kept * 25], totals dict)"""
    rec = np.frombuffer(np.ascontiguousarray(rec_bytes, np.uint8).tobytes(), RECORD)
    xy, what = classify(cam, opt, np.stack([rec["x"], rec["y"]], axis=1))
    keep = what == 0
    out = rec[keep].copy()
    out["x"] = xy[keep, 0]
    out["y"] = xy[keep, 1]
    totals = {"n_events": int(rec.size), "n_invalid": int((what == 1).sum()), "n_outside": int((what == 2).sum()), "n_kept": int(keep.sum())}
    return np.frombuffer(out.tobytes(), np.uint8), totals


def frame(cam, opt, pos_xy, neg_xy):
    """One window: the positive and negative points after the slicer -> (rgb [H, W, 3] uint8, totals (n_pos, n_neg, n_invalid,
    n_outside)).  Green where a valid negative point lands, else red where a valid positive one does."""
    W, H = int(opt["out_width"]), int(opt["out_height"])
    rgb = np.zeros((H, W, 3), np.uint8)
    tot = [0, 0, 0, 0]
    marks = []
    for pol, pts in enumerate((pos_xy, neg_xy)):
        pts = np.asarray(pts, np.float64).reshape(-1, 2)
        xy, what = classify(cam, opt, pts)
        tot[pol] = int((what == 0).sum())
        tot[2] += int((what == 1).sum())
        tot[3] += int((what == 2).sum())
        marks.append(xy[what == 0].astype(np.int64))
    rgb[marks[0][:, 1], marks[0][:, 0]] = (255, 0, 0)
    rgb[marks[1][:, 1], marks[1][:, 0]] = (0, 255, 0)
    return rgb, tuple(tot)
