"""CPU: the residual header (eventcalib_amd/csrc/spline_residual.hpp, compiled for the host with g++ -ffp-contract=off) AND the
oracle's dual-number functions (oracle/solver_oracle.cpp) at the edges of the residual's branches, each against a 60-digit mpmath
restatement of the same formulas WITHOUT any series branch, Jacobian rows by central differences at h = 1e-25 in the tangent
space (q_j <- exp(d) (x) q_j with Eigen's full-angle Plus for the quaternion blend, q_j <- q_j (x) exp(d) for the SO3 spline).

This is what qualifies the oracle as the reference of tests/test_gpu_solver_edges.py: before its fisheye functor took the series
of tan(r poly) / r near r = 0 it returned NaN for a pixel exactly on the principal point (it divided by r).

Cases (tests/synth_solver_edges.py: ANGLES, PIXEL_OFFSETS):
  * angles   every relative angle of ANGLES (0 .. 3.0 rad, random directions) on each of the three relative rotations alone
             (the other two at 0.05 rad) and on all three, SO3 spline, basis values of a mid-span time; all three again with basis
             values near 0 and near 1 (beta * d crosses the thresholds of so3_exp / so3_rotate / so3_jl on its own), with the
             fisheye camera, and through the quaternion blend;
  * flip     one control point negated (-q), each of the four, both rotation modes;
  * pixels   the pixel at (cx, cy) and PIXEL_OFFSETS away from it, both cameras, both rotation modes.
A direction is redrawn while the ray runs within ~12 degrees of the board's plane (|Y_z| < 0.2): there the residual is singular
(depth = -T_z / Y_z) and amplifies rounding by 1 / Y_z^2, which is not the edge under test.

Tolerances (those of test_per_residual_rows_match_dual_numbers / test_fisheye_rows_match_dual_numbers): 1e-11 absolute on r (cm),
1e-11 on the row relative to its largest entry, 1e-10 on the row with the fisheye camera.
Measured on the host (x86-64, g++ -O2 -ffp-contract=off), 140 cases, ~8 s of mpmath; the table by family is in
design/08_solver.md, "Edges of the residual's branches":
  * product header: worst |dr| 1.8e-13 (3.0 rad), worst row 5.5e-13 at 1.1e-4 rad, just above the 1e-8 threshold of so3_jl /
    so3_jinv ((1 - cos t) / t^2 cancels; an earlier run of this comparison saw 3.8e-13 there), ~1e-15 elsewhere;
  * oracle: worst |dr| 2.1e-13 (3.0 rad), worst row 3.1e-15; finite and within 6.5e-16 on the row at the principal point."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import synth_solver as SV
import synth_solver_edges as E

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "residual_edges_host.cpp")
TOL_R, TOL_ROW, TOL_ROW_FISHEYE = 1e-11, 1e-11, 1e-10
H_FD = "1e-25"


# ---- the 60-digit restatement ----
def _qmul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def _norm3(v):
    return mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _so3_exp(w):
    th = _norm3(w)
    if th == 0:
        return [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)]
    s = mp.sin(th / 2) / th
    return [s * w[0], s * w[1], s * w[2], mp.cos(th / 2)]


def _so3_log(q):
    """rotation vector with angle 2 atan(|v| / w) in (-pi, pi): the same rotation for q and -q"""
    n = _norm3(q)
    if n == 0:
        return [mp.mpf(0)] * 3
    f = 2 * mp.atan(n / q[3]) / n
    return [f * q[0], f * q[1], f * q[2]]


def _plus_blend(q, d):
    """EigenQuaternionParameterization::Plus: exp(d) (x) q with the FULL angle |d|"""
    nd = _norm3(d)
    if nd == 0:
        return list(q)
    s = mp.sin(nd) / nd
    return _qmul([s * d[0], s * d[1], s * d[2], mp.cos(nd)], q)


def _plus_so3(q, d):
    """LocalParameterizationSO3::Plus: q (x) exp(d)"""
    return _qmul(q, _so3_exp(d))


def mp_residual(case, z=None):
    """the residual of `case` at the tangent offset z (33 mpf: intrinsics | 4 x 3 rotation | 4 x 3 translation)"""
    f = lambda a: [mp.mpf(float(v)) for v in np.asarray(a, np.float64).ravel()]
    intr, qf, tf, b, obs, lm = f(case["intr"]), f(case["q"]), f(case["t"]), f(case["b"]), f(case["obs"]), f(case["lm"])
    q = [qf[4 * j: 4 * j + 4] for j in range(4)]
    t = [tf[3 * j: 3 * j + 3] for j in range(4)]
    if z is not None:
        intr = [intr[i] + z[i] for i in range(9)]
        plus = _plus_so3 if case["so3"] else _plus_blend
        q = [plus(q[j], z[9 + 3 * j: 12 + 3 * j]) if any(v != 0 for v in z[9 + 3 * j: 12 + 3 * j]) else q[j] for j in range(4)]
        t = [[t[j][k] + z[21 + 3 * j + k] for k in range(3)] for j in range(4)]
    if case["so3"]:
        beta = [b[1] + b[2] + b[3], b[2] + b[3], b[3]]
        Q = q[0]
        for j in range(1, 4):
            inv = [-q[j - 1][0], -q[j - 1][1], -q[j - 1][2], q[j - 1][3]]
            d = _so3_log(_qmul(inv, q[j]))
            Q = _qmul(Q, _so3_exp([beta[j - 1] * v for v in d]))
    else:
        v = [sum(b[j] * q[j][k] for j in range(4)) for k in range(4)]
        n = mp.sqrt(sum(x * x for x in v))
        Q = [x / n for x in v]
    T = [sum(b[j] * t[j][k] for j in range(4)) for k in range(3)]
    x, y = (obs[0] - intr[2]) / intr[0], (obs[1] - intr[3]) / intr[1]
    r2 = x * x + y * y
    poly = 1 + r2 * (intr[4] + r2 * (intr[5] + r2 * (intr[6] + r2 * (intr[7] + r2 * intr[8]))))
    c = poly
    if case["fisheye"]:
        r = mp.sqrt(r2)
        c = mp.tan(r * poly) / r if r != 0 else poly     # (the limit at r = 0, not a series: tan(r poly) / r -> poly)
    p = [x * c, y * c, mp.mpf(1)]
    u, w = Q[:3], Q[3]
    cxp = [u[1] * p[2] - u[2] * p[1], u[2] * p[0] - u[0] * p[2], u[0] * p[1] - u[1] * p[0]]
    udp = u[0] * p[0] + u[1] * p[1] + u[2] * p[2]
    udu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    Y = [p[k] + 2 * w * cxp[k] + 2 * (u[k] * udp - p[k] * udu) for k in range(3)]
    s = -T[2] / Y[2]
    Xw = [T[k] + s * Y[k] for k in range(3)]
    return mp.sqrt(sum((Xw[k] - lm[k]) ** 2 for k in range(3))) - mp.mpf(float(case["radius"]))


def mp_row(case):
    h = mp.mpf(H_FD)
    zero = [mp.mpf(0)] * 33
    r = mp_residual(case)
    J = []
    for i in range(33):
        zp, zm = list(zero), list(zero)
        zp[i], zm[i] = h, -h
        J.append((mp_residual(case, zp) - mp_residual(case, zm)) / (2 * h))
    return r, J


# ---- the cases ----
def _ray_y2(case):
    """Y_z of the case's ray in f64 (the guard against rays along the board)"""
    b, q = np.asarray(case["b"]), np.asarray(case["q"]).reshape(4, 4)
    if case["so3"]:
        Q = SV.so3_spline_pose(q, b)
    else:
        Q = b @ q
        Q = Q / np.linalg.norm(Q)
    intr = case["intr"]
    x, y = (case["obs"][0] - intr[2]) / intr[0], (case["obs"][1] - intr[3]) / intr[1]
    return SV.quat_rotate(Q, np.array([x, y, 1.0]))[2]


B_MID = SV.basis(np.array([0, 0, 0, 0, 0.21, 0.48, 0.77, 1, 1, 1, 1.0]), 4, 0.33)
B_NEAR1 = np.array([1e-3, 2e-3, 3e-3, 1.0 - 6e-3])       # cumulative basis 0.999, 0.997, 0.994
B_NEAR0 = np.array([1.0 - 6e-3, 3e-3, 2e-3, 1e-3])       # cumulative basis 6e-3, 3e-3, 1e-3


def _case(rng, family, name, so3, fisheye, angles, b, flip=None, pixel_offset=None):
    intr = (SV.GT_INTR_FISHEYE if fisheye else SV.GT_INTR).copy()
    t = E.translations(4, rng)
    lm = SV.landmarks()[int(rng.integers(0, 36))]
    for _ in range(200):
        q = E.rotation_chain(4, angles, rng)
        if flip is not None:
            q[flip] = -q[flip]
        if pixel_offset is None:
            obs = E.random_pixels(1, rng)[0]
        else:
            a = rng.uniform(0, 2 * np.pi)
            obs = np.array([intr[2] + pixel_offset * np.cos(a), intr[3] + pixel_offset * np.sin(a)]) if pixel_offset else intr[2:4].copy()
        case = dict(family=family, name=name, so3=bool(so3), fisheye=bool(fisheye), intr=intr, q=q, t=t, b=np.asarray(b, np.float64),
                    obs=obs, lm=lm, radius=E.RADIUS)
        if abs(_ray_y2(case)) >= 0.2:
            return case
    raise AssertionError("no well-conditioned direction found for " + name)


def build_cases():
    rng = np.random.default_rng(20240)
    cases = []
    for a in E.ANGLES:
        for which in (0, 1, 2, None):
            ang = [a if which in (None, j) else 0.05 for j in range(3)]
            cases.append(_case(rng, "angles", "so3 angle %g on %s" % (a, "all" if which is None else "d%d" % (which + 1)), True, False, ang, B_MID))
        cases.append(_case(rng, "angles beta->1", "so3 angle %g basis near 1" % a, True, False, a, B_NEAR1))
        cases.append(_case(rng, "angles beta->0", "so3 angle %g basis near 0" % a, True, False, a, B_NEAR0))
        cases.append(_case(rng, "angles fisheye", "so3 fisheye angle %g" % a, True, True, a, B_MID))
        cases.append(_case(rng, "angles blend", "blend angle %g" % a, False, False, a, B_MID))
    for so3 in (False, True):
        for j in range(4):
            # (blend: a control point and its negative on either side of the blend pull the sum towards 0: 0.05 rad keeps it a rotation)
            cases.append(_case(rng, "flip", "%s -q%d" % ("so3" if so3 else "blend", j), so3, False, 0.05, B_NEAR1 if j == 3 else (B_NEAR0 if j == 0 else B_MID),
                               flip=j))
    for so3 in (False, True):
        for fisheye in (False, True):
            for off in E.PIXEL_OFFSETS:
                cases.append(_case(rng, "pixels fisheye" if fisheye else "pixels pinhole", "%s %s offset %g px" % ("so3" if so3 else "blend",
                                   "fisheye" if fisheye else "pinhole", off), so3, fisheye, 0.05, B_MID, pixel_offset=off))
    return cases


def _hex_line(case):
    vals = np.concatenate([case["intr"], case["q"].ravel(), case["t"].ravel(), case["b"], case["obs"], case["lm"], [case["radius"]]])
    assert vals.shape[0] == 47
    return "%d %d %s" % (case["so3"], case["fisheye"], " ".join(float(v).hex() for v in vals))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    O.lib()                                          # (builds oracle/liboracle.so when it is absent)
    exe = str(tmp_path_factory.mktemp("edges") / "residual_edges_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, SRC, "-L" + O.ORACLE_DIR, "-loracle",
                           "-Wl,-rpath," + O.ORACLE_DIR])
    cases = build_cases()
    out = subprocess.run([exe], input="\n".join(_hex_line(c) for c in cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.split("\n")
    assert len([ln for ln in lines if ln]) == 2 * len(cases)
    old = mp.dps
    mp.dps = 60
    try:
        res = []
        for i, c in enumerate(cases):
            r_ref, J_ref = mp_row(c)
            scale = max(abs(v) for v in J_ref)
            entry = dict(case=c, tol_row=TOL_ROW_FISHEYE if c["fisheye"] else TOL_ROW)
            for tag, ln in (("P", lines[2 * i]), ("O", lines[2 * i + 1])):
                tok = ln.split()
                assert tok[0] == tag
                vals = [float.fromhex(v) for v in tok[1:]]
                assert len(vals) == 34
                finite = bool(np.isfinite(vals).all())
                entry[tag] = dict(finite=finite,
                                  err_r=float(abs(mp.mpf(vals[0]) - r_ref)) if finite else np.inf,
                                  err_row=float(max(abs(mp.mpf(vals[1 + k]) - J_ref[k]) for k in range(33)) / scale) if finite else np.inf)
            res.append(entry)
    finally:
        mp.dps = old
    # the worst error of every family: what design/08_solver.md records
    for tag, who in (("P", "product header"), ("O", "oracle")):
        for fam in sorted({e["case"]["family"] for e in res}):
            sel = [e[tag] for e in res if e["case"]["family"] == fam]
            print("%-14s %-16s n=%2d worst |dr| %.2e  worst row %.2e" % (who, fam, len(sel), max(s["err_r"] for s in sel), max(s["err_row"] for s in sel)))
    return res


def _failures(results, tag):
    return [(e["case"]["name"], e[tag]["err_r"], e[tag]["err_row"]) for e in results
            if not (e[tag]["finite"] and e[tag]["err_r"] <= TOL_R and e[tag]["err_row"] <= e["tol_row"])]


def test_the_sweep_covers_the_issue(results):
    fam = {}
    for e in results:
        fam[e["case"]["family"]] = fam.get(e["case"]["family"], 0) + 1
    n = len(E.ANGLES)
    assert fam == {"angles": 4 * n, "angles beta->1": n, "angles beta->0": n, "angles fisheye": n, "angles blend": n, "flip": 8,
                   "pixels pinhole": 2 * len(E.PIXEL_OFFSETS), "pixels fisheye": 2 * len(E.PIXEL_OFFSETS)}
    # the thresholds are straddled as meant: r2 on either side of 1e-16 and of 1e-8
    fx = SV.GT_INTR_FISHEYE[0]
    r2 = [(o / fx) ** 2 for o in E.PIXEL_OFFSETS]
    assert r2[2] < 1e-16 < r2[3] and r2[4] < 1e-8 < r2[5]


def test_product_header_matches_mpmath_at_every_edge(results):
    bad = _failures(results, "P")
    assert not bad, bad


def test_oracle_matches_mpmath_at_every_edge(results):
    bad = _failures(results, "O")
    assert not bad, bad


def test_oracle_is_finite_on_the_principal_point(results):
    """the case that returned NaN before the fisheye functor took its series near r = 0"""
    hit = [e for e in results if e["case"]["fisheye"] and e["case"]["name"].endswith("offset 0 px")]
    assert len(hit) == 2
    for e in hit:
        assert e["O"]["finite"] and e["O"]["err_r"] <= TOL_R and e["O"]["err_row"] <= TOL_ROW_FISHEYE, (e["case"]["name"], e["O"])
