"""Synthetic asymmetric circle boards of any shape: the ground truth the grid finder is tested against (numpy float64, CPU only,
no code shared with the library).

Convention (include/ecal.h, the reference's EventCalibIni.cpp:102-106): grid index i*cols + j is the model point
((2j + i%2) s, i s), i = row, j = column."""
import numpy as np


def model_points(rows, cols, s=1.0):
    """[rows*cols, 2]: index i*cols + j -> ((2j + i%2) s, i s)."""
    i, j = np.divmod(np.arange(rows * cols), cols)
    return np.stack([(2 * j + i % 2) * float(s), i * float(s)], axis=1).astype(np.float64)


def self_symmetries(rows, cols):
    """The index permutations p (p[m] = model point that model point m lands on) under which the model point set maps onto
    itself by an orientation-preserving rigid motion.  Brute force on the point set: such a motion keeps the centroid, so it is
    a turn about it, and a finite planar point set on this lattice admits quarter turns at most — all four are tried.  The
    identity is always the first entry."""
    p = model_points(rows, cols)
    c = p.mean(axis=0)
    out = []
    for q in range(4):
        co, si = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][q]
        t = (p - c) @ np.array([[co, si], [-si, co]]) + c          # every point turned by q quarter turns about the centroid
        d = np.abs(t[:, None, :] - p[None, :, :]).max(axis=2)      # [m, m']
        hit = d < 1e-9
        if hit.any(axis=1).all():
            perm = hit.argmax(axis=1)
            if len(set(perm.tolist())) == len(p):
                out.append(perm.astype(np.int64))
    return out


def nn_step(pts):
    """mean nearest-neighbour distance of a point set"""
    d = np.linalg.norm(pts[:, None, :] - pts[None, :, :], axis=2)
    np.fill_diagonal(d, np.inf)
    return float(d.min(axis=1).mean())


def views(rows, cols, image_wh=None, step_px=40.0, tilt_deg=0.0, roll_deg=0.0, seed=0, distance=4.0):
    """The board's circle centres in a pinhole camera's image, [M, 2] float64, seen from the FRONT (model -> image with positive
    determinant: image x to the right, y down, as the model's).  The camera sits `distance` board diagonals from the board's
    centre with its optical axis through it, tilted off the board's normal by tilt_deg about an in-plane axis whose azimuth is
    drawn from `seed`, and turned about the optical axis by roll_deg.  The image is scaled so that the mean nearest-neighbour
    distance of the projected circles is step_px, and the box of the projections is centred in image_wh (None: an image that
    holds the board with four steps to spare on every side)."""
    rng = np.random.default_rng(seed)
    p = model_points(rows, cols)
    ctr = 0.5 * (p.min(axis=0) + p.max(axis=0))
    P = np.concatenate([p - ctr, np.zeros((len(p), 1))], axis=1)                # board in the plane z = 0, centre at the origin
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    a, az, ro = np.deg2rad(tilt_deg), rng.uniform(0.0, 2.0 * np.pi), np.deg2rad(roll_deg)
    zc = np.array([np.sin(a) * np.cos(az), np.sin(a) * np.sin(az), np.cos(a)])  # optical axis; the camera looks along +z at the board
    xc = np.array([1.0, 0.0, 0.0]) - zc[0] * zc
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    xc, yc = np.cos(ro) * xc + np.sin(ro) * yc, -np.sin(ro) * xc + np.cos(ro) * yc
    C = -distance * diag * zc
    Q = P - C
    Z = Q @ zc
    assert (Z > 0).all()
    uv = np.stack([(Q @ xc) / Z, (Q @ yc) / Z], axis=1)
    uv *= step_px / nn_step(uv)
    lo, hi = uv.min(axis=0), uv.max(axis=0)
    wh = (hi - lo) + 8.0 * step_px if image_wh is None else np.asarray(image_wh, np.float64)
    return uv - 0.5 * (lo + hi) + 0.5 * wh


def ring_clutter(pts, k, min_steps, rng):
    """k false candidates on a ring around the board, [k, 2]: evenly spread in angle from a random first angle (so their centroid
    is the ring's centre, the board's own centroid), every one at least min_steps lattice steps (mean nearest-neighbour distances
    of pts) from every circle and from the other false ones."""
    if k <= 0:
        return np.zeros((0, 2))
    c = pts.mean(axis=0)
    gap = float(min_steps) * nn_step(pts)
    R = float(np.linalg.norm(pts - c, axis=1).max()) + gap
    if k > 1:
        R = max(R, 1.001 * gap / (2.0 * np.sin(np.pi / k)))                    # chord between neighbours on the ring >= gap
    ang = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.arange(k) / k
    return c + R * np.stack([np.cos(ang), np.sin(ang)], axis=1)


def expected_orders(perm, rows, cols):
    """The acceptable `order` vectors for a candidate list that is all[perm] with the board's circles all[:M] in model order:
    circle k sits at position argsort(perm)[k]; every self-symmetry of the board gives one more valid assignment."""
    inv = np.argsort(np.asarray(perm))
    return [inv[sym].astype(np.int64) for sym in self_symmetries(rows, cols)]
