"""Edge problems of the continuous-time solve, built from explicit lists (test infrastructure, plain numpy on synth_solver).

synth_solver.make_problem draws its event times uniformly and moves the camera smoothly, so no residual of it sits on a knot,
no two neighbouring rotation control points are closer than 0.01 rad and no pixel is near the principal point.  The builders
here put the data exactly there: times given one by one (on knots, one ulp beside them), control points a prescribed angle
apart (down to 0, and sign-flipped), pixels at a prescribed offset from (cx, cy), spans with a prescribed number of residuals.
The observations are NOT projections of the board: the residuals are of the order of centimetres, which is what a residual /
Jacobian comparison needs and no more."""
import ctypes

import numpy as np

import synth_solver as SV

RADIUS = SV.RADIUS

# the relative angles (rad) between neighbouring rotation control points: the small-angle branches of spline_residual.hpp are
# so3_log n2 < 1e-20 (angle < 2e-10), so3_exp t2 < 1e-20 (beta * angle < 1e-10), so3_rotate t2 < 1e-12 (1e-6), so3_jl / so3_jinv
# t2 < 1e-8 (1e-4); the sweep ends at 3.0 rad (so3_log folds at pi, where the host code itself loses accuracy)
ANGLES = (0.0, 1e-12, 0.9e-10, 1.1e-10, 1e-8, 0.9e-6, 1.1e-6, 0.9e-4, 1.1e-4, 1e-3, 0.1, 1.0, 3.0)
# pixel offsets (px) from the principal point: r2 = (off / fx)^2 straddles 1e-16 (3e-6 | 4e-6 px) and 1e-8 (0.03 | 0.04 px) at fx = 359.67
PIXEL_OFFSETS = (0.0, 1e-9, 3e-6, 4e-6, 0.03, 0.04, 1.0)

# the camera looks down the board's normal from ~66 cm, rolled by 90 degrees and tilted a little (xyzw)
BASE_Q = np.array([0.03, -0.02, np.sin(np.pi / 4), np.cos(np.pi / 4)])
BASE_Q = BASE_Q / np.linalg.norm(BASE_Q)


def so3_exp(w):
    """rotation vector -> unit quaternion (xyzw), the closed form at every angle but 0 (sin(x) / x is exact to rounding in f64)"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(0.5 * th) / th * w, [np.cos(0.5 * th)]])


def random_direction(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def rotation_chain(n_cp, angles, rng, base=BASE_Q, directions=None):
    """n_cp unit quaternions with q_j = q_{j-1} (x) exp(angles[j-1] * direction_j): neighbouring control points exactly the given
    angle apart up to the rounding of the product (1e-16 on a component).  angles: one value, or n_cp - 1 of them.  An angle of 0
    repeats the control point bit for bit."""
    ang = np.broadcast_to(np.asarray(angles, np.float64), (n_cp - 1,))
    q = np.zeros((n_cp, 4))
    q[0] = base
    for j in range(1, n_cp):
        d = random_direction(rng) if directions is None else np.asarray(directions[j - 1], np.float64)
        q[j] = q[j - 1].copy() if ang[j - 1] == 0.0 else SV.quat_mul(q[j - 1], so3_exp(ang[j - 1] * d))
        q[j] /= np.linalg.norm(q[j])
    return q


def translations(n_cp, rng=None, still=False):
    """translation control points ~66 cm above the board (synth_solver's path), optionally all equal (a camera that stands still)"""
    t = SV.gt_control_points(n_cp, 5.0, 5.5)[1]
    if still:
        t = np.repeat(t[:1], n_cp, axis=0)
    if rng is not None:
        t = t + 0.3 * rng.normal(size=t.shape)
    return t


def params(intr, q, t):
    return np.concatenate([np.asarray(intr, np.float64), np.asarray(q, np.float64).ravel(), np.asarray(t, np.float64).ravel()])


def jittered_knots(n_cp, t0, t1, rng):
    return SV.clamped_knots(n_cp, t0, t1, rng)


def problem(knots, times, pixels, lm_ids, seg_cp_off=None, seg_ids=None, use_so3=False, fisheye=False, huber_a=0.2 * RADIUS):
    """A capi.Solver problem dict from explicit lists.  knots: one clamped knot vector, or a list of them (one per segment, then
    seg_cp_off and seg_ids say which residual belongs where).  times must ascend inside a segment."""
    if isinstance(knots, (list, tuple)):
        ncp = [len(k) - 4 for k in knots]
        kn = np.concatenate([np.asarray(k, np.float64) for k in knots])
        if seg_cp_off is None:
            seg_cp_off = np.concatenate([[0], np.cumsum(ncp)])
    else:
        kn = np.asarray(knots, np.float64)
        if seg_cp_off is None:
            seg_cp_off = [0, len(kn) - 4]
    times = np.asarray(times, np.float64).reshape(-1)
    n = times.shape[0]
    return dict(seg_cp_off=np.asarray(seg_cp_off, np.uint32), knots=kn, obs=np.asarray(pixels, np.float64).reshape(n, 2), time=times,
                lm_id=np.asarray(lm_ids, np.uint32).reshape(n), seg_id=None if seg_ids is None else np.asarray(seg_ids, np.uint32).reshape(n),
                landmarks=SV.landmarks(), circle_radius=RADIUS, huber_a=float(huber_a), use_so3=bool(use_so3), fisheye=bool(fisheye))


def random_pixels(n, rng):
    """pixels over the middle of a 346 x 260 sensor (the inverse polynomial of GT_INTR is meant for the sensor, not beyond it)"""
    return np.stack([rng.uniform(40, 306, n), rng.uniform(30, 230, n)], axis=1)


def random_landmarks(n, rng):
    return rng.integers(0, len(SV.landmarks()), n).astype(np.uint32)


def span_times(knots, n_cp, per_span, rng):
    """per_span times in every knot span, ascending: the span's first knot itself, one ulp above it, one ulp below its last knot
    (basis values at 0 and 1: the cumulative basis beta times the relative rotation crosses the small-angle thresholds on its
    own), the rest uniform; the segment's last knot closes the list."""
    out = []
    for span in range(3, n_cp):
        a, b = knots[span], knots[span + 1]
        fixed = [a, np.nextafter(a, np.inf), np.nextafter(b, -np.inf)]
        out.extend(fixed + list(rng.uniform(a, b, max(per_span - len(fixed), 0))))
    out.append(knots[n_cp])
    return np.sort(np.array(out))


def knot_times(knots, n_cp, repeat=3):
    """every distinct knot of the segment `repeat` times over — the first, every interior one with the doubles just below and
    above it, the last — ascending"""
    out = [knots[3]] * repeat
    for k in range(4, n_cp):
        for v in (np.nextafter(knots[k], -np.inf), knots[k], np.nextafter(knots[k], np.inf)):
            out += [v] * repeat
    out += [knots[n_cp]] * repeat
    return np.array(out)


def expected_chunks(m):
    """the number of chunks ecal_solver_create cuts a span of m residuals into: parts = ceil(m / 16384) equal parts, each
    rounded up to whole batches of 256 rows"""
    if m == 0:
        return 0
    parts = -(-m // 16384)
    per = -(-(-(-m // parts)) // 256) * 256
    return -(-m // per)


def counted_span_times(knots, n_cp, counts, rng):
    """counts[i] times strictly inside span 3 + i (ascending): spans with a prescribed number of residuals, 0 included"""
    assert len(counts) == n_cp - 3
    out = []
    for i, m in enumerate(counts):
        a, b = knots[3 + i], knots[4 + i]
        out.append(np.sort(rng.uniform(a + 0.01 * (b - a), b - 0.01 * (b - a), m)))
    return np.concatenate(out) if out else np.zeros(0)


def ray_yz(prob, y):
    """Y_z of every residual's ray (one segment, f64): the component of the rotated viewing ray along the board's normal.  The
    residual divides by it (depth = -T_z / Y_z), so a test of something else keeps |Y_z| away from 0."""
    n_cp = int(prob["seg_cp_off"][-1])
    q = np.asarray(y[9:9 + 4 * n_cp]).reshape(n_cp, 4)
    out = np.zeros(len(prob["time"]))
    for k, u in enumerate(prob["time"]):
        sp = SV.find_span(prob["knots"], n_cp, u)
        b = SV.basis(prob["knots"], sp, u)
        if prob.get("use_so3"):
            Q = SV.so3_spline_pose(q[sp - 3: sp + 1], b)
        else:
            Q = b @ q[sp - 3: sp + 1]
            nq = np.linalg.norm(Q)
            if nq < 0.2:             # (a blend through a sign-flipped control point: the normalisation itself is singular)
                out[k] = 0.0
                continue
            Q = Q / nq
        x, yy = (prob["obs"][k, 0] - y[2]) / y[0], (prob["obs"][k, 1] - y[3]) / y[1]
        out[k] = SV.quat_rotate(Q, np.array([x, yy, 1.0]))[2]
    return out


# ---- the oracle's dual numbers, residual by residual ----
_dp = ctypes.POINTER(ctypes.c_double)


def oracle_rows(prob, y):
    """(r [n], J [n, 33], cp0 [n]) of every residual from oracle_find_span / oracle_basis / oracle_residual*_cam (forward-mode dual
    numbers through the restated functor and local parameterisation); cp0 counts over all segments like the product's."""
    import oracle_lib as O
    L = O.lib()
    L.oracle_find_span.argtypes = [_dp, ctypes.c_uint32, ctypes.c_double]
    L.oracle_find_span.restype = ctypes.c_uint32
    L.oracle_basis.argtypes = [_dp, ctypes.c_uint32, ctypes.c_double, _dp]
    L.oracle_basis.restype = None
    fn = L.oracle_residual_so3_cam if prob.get("use_so3") else L.oracle_residual_cam
    fn.argtypes = [_dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_double, _dp, _dp, ctypes.c_int]
    fn.restype = ctypes.c_double
    p = lambda a: a.ctypes.data_as(_dp)
    cp_off = np.asarray(prob["seg_cp_off"], np.int64)
    n_cp = int(cp_off[-1])
    y = np.ascontiguousarray(y, np.float64)
    intr = y[:9].copy()
    q = y[9:9 + 4 * n_cp].reshape(n_cp, 4)
    t = y[9 + 4 * n_cp:].reshape(n_cp, 3)
    n = len(prob["time"])
    seg = np.zeros(n, np.int64) if prob.get("seg_id") is None else np.asarray(prob["seg_id"], np.int64)
    lms = np.ascontiguousarray(prob["landmarks"], np.float64).reshape(-1, 3)
    r, J, cp0 = np.zeros(n), np.zeros((n, 33)), np.zeros(n, np.uint32)
    for k in range(n):
        g = int(seg[k])
        ncp_g = int(cp_off[g + 1] - cp_off[g])
        ko = int(cp_off[g]) + 4 * g
        kn = np.ascontiguousarray(prob["knots"][ko: ko + ncp_g + 4], np.float64)
        u = float(prob["time"][k])
        span = int(L.oracle_find_span(p(kn), ncp_g, u))
        c0 = int(cp_off[g]) + span - 3
        b4 = np.zeros(4)
        L.oracle_basis(p(kn), span, u, p(b4))
        q4 = np.ascontiguousarray(q[c0:c0 + 4]).copy()
        t4 = np.ascontiguousarray(t[c0:c0 + 4]).copy()
        obs = np.ascontiguousarray(prob["obs"][k], np.float64).copy()
        lm = lms[int(prob["lm_id"][k])].copy()
        J33 = np.zeros(33)
        r[k] = fn(p(intr), p(q4), p(t4), p(b4), p(obs), p(lm), float(prob["circle_radius"]), None, p(J33), int(bool(prob.get("fisheye"))))
        J[k] = J33
        cp0[k] = c0
    return r, J, cp0
