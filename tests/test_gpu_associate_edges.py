"""GPU parity at the association kernel's edges (ecal_associate.hip), bit for bit against the brute-force oracle
(oracle/associate_oracle.cpp: every event against every keyframe and every circle): the plain path, the staging threshold,
arbitrary event order, exact ties and strict bounds, the scan's carry between rounds, sizes below a block, the keyframe
count the wave search sees, range tables beyond LDS and the host form.  No tolerance anywhere: the arithmetic is the same
f64 without contraction, the outputs are copies and indices.

Every input is built so that its branch is reached by construction, and `_plan` (the kernel's staging decision restated in
numpy) or the oracle's own result asserts that it was.  Times are multiples of 2**-21 s and pixels, centres and radii are
integers, so distances and comparisons are exact and ties can be placed on purpose."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

# the kernel's constants (ecal_associate.hip): AS_T * AS_PER events a block, AS_KF_LDS keyframes / AS_CIRC_LDS circles per
# keyframe / AS_RNG_LDS time ranges a block stages in LDS
BLOCK, KF_LDS, CIRC_LDS, RNG_LDS = 1024, 6, 64, 32

H = 2.0 ** -20          # one event step in seconds: a block of consecutive events spans 2**-10 s
T0 = 3.0                # the stream's first time stamp (T0 + i * H is exact)
GUARD = 16              # records behind every output array that must stay untouched
F_SENT, I_SENT = -7.25, -77
RADIUS = 6.0
ECAL_OK, ECAL_ERR_INVALID, ECAL_ERR_RANGE = 0, -1, -6

_REC = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])
assert _REC.itemsize == 25


def _records(t, x, y):
    """The packed 25-byte event records (f64 t, f64 x, f64 y, u8 polarity) as a flat byte array."""
    r = np.zeros(len(t), _REC)
    r["t"], r["x"], r["y"] = t, x, y
    r["p"] = np.arange(len(t)) & 1
    return r.view(np.uint8).reshape(-1)


def _plan(t, kf, n_circ=36):
    """The kernel's staging decision for every 1024-event block -> (met [blocks], staged [blocks]).  Only there so that a test
    can assert that its INPUT reaches the branch it is named after."""
    t, kf = np.asarray(t, np.float64), np.asarray(kf, np.float64)
    n, K = len(t), len(kf)
    nb = (n + BLOCK - 1) // BLOCK
    pad = np.full(nb * BLOCK, np.nan)
    pad[:n] = t
    pad = pad.reshape(nb, BLOCK)
    with np.errstate(all="ignore"):
        block_min, block_max = np.fmin.reduce(pad, axis=1), np.fmax.reduce(pad, axis=1)   # (NaN times take no part)
    some = ~np.isnan(block_min)
    if K == 0:
        return np.zeros(nb, np.int64), np.zeros(nb, bool)
    a_lo = np.searchsorted(kf, np.where(some, block_min, 0.0), "left")
    a_hi = np.searchsorted(kf, np.where(some, block_max, 0.0), "left")
    k_first = np.maximum(a_lo - 1, 0)
    k_last = np.minimum(a_hi, K - 1)
    met = k_last - k_first + 1
    return met, some & (n_circ <= CIRC_LDS) & (met <= KF_LDS)


def _lattice(K, n_circ):
    """Circle table [K][n_circ][3] on an integer lattice: eight centres a row, 24 px apart, shifted by k % 3 px with the keyframe
    (so neighbouring keyframes give different answers), radius 6."""
    i, k = np.arange(n_circ), np.arange(K)
    c = np.empty((K, n_circ, 3))
    c[:, :, 0] = 20 + 24 * (i % 8)[None, :] + (k % 3)[:, None]
    c[:, :, 1] = 20 + 24 * (i // 8)[None, :]
    c[:, :, 2] = RADIUS
    return c


def _tie_pixel(circ, k, i):
    """A pixel that circle i ACCEPTS under keyframe k and that keyframe k + 1 REJECTS, for edge_tol = 6 (accepted: 0 < dist < 12):
    the centres move by +1, +1, -2 px from k to k + 1, so 11 px to the left (10 px to the right when k % 3 == 2) becomes 12 px
    there, from circle i and from its neighbour alike.  An event half way between k and k + 1 with this pixel is in the output
    exactly when the tie went to the smaller index."""
    cx, cy = circ[k, i, 0], circ[k, i, 1]
    return (cx - 11.0, cy) if k % 3 != 2 else (cx + 10.0, cy)


def _stream(n, kf_pos, n_circ, seed):
    """n events at T0 + i * H with random integer pixels, keyframes at T0 + kf_pos * H (kf_pos in event steps, multiples of
    0.5), the lattice table; an event that sits exactly half way between two keyframes gets a _tie_pixel.
    -> t, x, y, kf_time, circles, indices of the tie events"""
    rng = np.random.default_rng(seed)
    t = T0 + np.arange(n) * H
    x = rng.integers(5, 220, n).astype(np.float64)
    y = rng.integers(5, 200, n).astype(np.float64)
    kf_pos = np.asarray(kf_pos, np.float64)
    assert np.all(np.diff(kf_pos) > 0) and np.all(kf_pos * 2 == np.floor(kf_pos * 2))
    circ = _lattice(len(kf_pos), n_circ)
    ties = []
    for k, m in enumerate((kf_pos[:-1] + kf_pos[1:]) / 2):
        if m == np.floor(m) and 0 <= m < n:
            x[int(m)], y[int(m)] = _tie_pixel(circ, k, (7 * k) % n_circ)
            ties.append(int(m))
    return t, x, y, T0 + kf_pos * H, circ, np.array(ties, np.int64)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import eventcalib_amd
    ctx = eventcalib_amd.Context(0)
    yield ctx, torch
    ctx.close()


def _launch(gpu, rec, kt, circ, gate, max_dt, tol):
    """One association on the device.  gate = (t_min, t_max), or an array [R][2] of ranges (ecal_associate_ranges_dev).  The count
    word starts as 0xDEADBEEF, the outputs are filled with sentinels and everything from record `count` on, the GUARD records
    behind the arrays included, must come back untouched."""
    ctx, torch = gpu
    n = rec.size // 25
    K, nc = (circ.shape[0], circ.shape[1]) if len(kt) else (0, 36)
    ranges = None if isinstance(gate, tuple) else np.ascontiguousarray(gate, np.float64).reshape(-1, 2)
    d_ev = torch.from_numpy(rec).cuda()
    d_kt = torch.from_numpy(np.ascontiguousarray(kt, np.float64)).cuda()
    d_ci = torch.from_numpy(np.ascontiguousarray(circ, np.float64)).cuda()
    obs = torch.full((n + GUARD, 2), F_SENT, dtype=torch.float64, device="cuda")
    tm = torch.full((n + GUARD,), F_SENT, dtype=torch.float64, device="cuda")
    lm = torch.full((n + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    sg = torch.full((n + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), 0xDEADBEEF - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if ranges is None:
        ctx.associate_dev(d_ev.data_ptr(), n, d_kt.data_ptr(), d_ci.data_ptr(), K, nc, gate[0], gate[1], max_dt, tol,
                          obs.data_ptr(), tm.data_ptr(), lm.data_ptr(), cnt.data_ptr(), 0)
    else:
        d_rg = torch.from_numpy(ranges).cuda()
        ctx.associate_ranges_dev(d_ev.data_ptr(), n, d_kt.data_ptr(), d_ci.data_ptr(), K, nc, d_rg.data_ptr(), len(ranges), max_dt, tol,
                                 obs.data_ptr(), tm.data_ptr(), lm.data_ptr(), sg.data_ptr(), cnt.data_ptr(), 0)
    torch.cuda.synchronize()
    m = int(cnt.item()) & 0xFFFFFFFF
    assert m <= n, "count %#x" % m
    assert bool((obs[m:] == F_SENT).all()) and bool((tm[m:] == F_SENT).all()) and bool((lm[m:] == I_SENT).all()), "written beyond the count"
    assert bool((sg[m if ranges is not None else 0:] == I_SENT).all())
    return dict(m=m, obs=obs[:m].cpu().numpy(), time=tm[:m].cpu().numpy(), lm=lm[:m].cpu().numpy().astype(np.uint32),
                seg=sg[:m].cpu().numpy().astype(np.uint32) if ranges is not None else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_same(got, want, seg=None):
    """bit equality of the count, obs, time, lm_id (and seg_id) with the oracle's (obs, time, lm_id)"""
    assert got["m"] == len(want[1]), (got["m"], len(want[1]))
    assert np.array_equal(_bits(got["obs"]), _bits(want[0]))
    assert np.array_equal(_bits(got["time"]), _bits(want[1]))
    assert np.array_equal(got["lm"], want[2])
    if seg is not None:
        assert np.array_equal(got["seg"], seg)


def _assert_ties_taken(t, ties, want):
    """the oracle put every tie event into its output (so the tie went to the smaller index there: _tie_pixel) — a kernel that
    sends one to the larger index drops it and misses the count"""
    assert len(ties) >= 3 and np.isin(t[ties], want[1]).all()


# ---- 1. the plain path by circle count -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sparse_kf():
    """40 000 time-ordered events, a keyframe every four blocks (at 2000 + 4096 j events: the half-way points are events)"""
    n = 40000
    return n, 2000.0 + 4096.0 * np.arange(-1, 11)


def test_circle_count_decides_the_path(gpu, sparse_kf):
    """36 circles are staged; the same table padded to 65 per keyframe (29 circles at (1e6, 1e6), never nearest) sends every block
    the plain way (n_circles > AS_CIRC_LDS): both equal the oracle and each other."""
    n, kf_pos = sparse_kf
    t, x, y, kt, circ, ties = _stream(n, kf_pos, 36, 41)
    rec = _records(t, x, y)
    gate, max_dt, tol = (t[0], t[-1]), 2100 * H, 6.0
    assert _plan(t, kt, 36)[1].all() and not _plan(t, kt, CIRC_LDS + 1)[1].any()
    want = O.associate(rec, kt, circ, gate[0], gate[1], max_dt, tol)
    assert 0.15 * n < len(want[1]) < 0.9 * n
    _assert_ties_taken(t, ties, want)
    staged = _launch(gpu, rec, kt, circ, gate, max_dt, tol)
    _assert_same(staged, want)
    wide = np.empty((len(kt), CIRC_LDS + 1, 3))
    wide[:, :36] = circ
    wide[:, 36:] = (1.0e6, 1.0e6, 1.0)
    want_wide = O.associate(rec, kt, wide, gate[0], gate[1], max_dt, tol)
    assert all(np.array_equal(a, b) for a, b in zip(want_wide, want))
    plain = _launch(gpu, rec, kt, wide, gate, max_dt, tol)
    _assert_same(plain, want_wide)
    _assert_same(plain, (staged["obs"], staged["time"], staged["lm"]))


@pytest.mark.parametrize("n_circ", [1, CIRC_LDS])
def test_circle_count_one_and_the_fullest_staged_table(gpu, sparse_kf, n_circ):
    """n_circles = 64 = AS_CIRC_LDS is the fullest s_circ (still staged), n_circles = 1 the smallest table"""
    n, kf_pos = sparse_kf
    t, x, y, kt, circ, ties = _stream(n, kf_pos, n_circ, 42)
    rec = _records(t, x, y)
    assert _plan(t, kt, n_circ)[1].all()
    want = O.associate(rec, kt, circ, t[0], t[-1], 2100 * H, 6.0)
    assert 100 < len(want[1]) < n
    _assert_ties_taken(t, ties, want)
    _assert_same(_launch(gpu, rec, kt, circ, (t[0], t[-1]), 2100 * H, 6.0), want)


# ---- 2. the staging threshold by time span -------------------------------------------------------------------------------

def _dense_kf(n):
    """A keyframe every 227 events (a block's span / 4.5), off the events' lattice (x.5): a block's span then holds four or five
    of them, so it meets six (the fullest s_kt: staged) or seven (the first count that must go the plain way); the first block,
    before which there is no keyframe, meets five.  Every half-way point (227 is odd) is an event."""
    return 130.5 + 227.0 * np.arange(0, int(np.ceil(n / 227.0)) + 1)


@pytest.fixture(scope="module")
def dense():
    n = 60 * BLOCK
    t, x, y, kt, circ, ties = _stream(n, _dense_kf(n), 36, 43)
    return dict(n=n, t=t, x=x, y=y, kt=kt, circ=circ, ties=ties, max_dt=120 * H, tol=6.0)


def test_blocks_on_both_sides_of_the_staging_threshold(gpu, dense):
    d = dense
    met, staged = _plan(d["t"], d["kt"])
    assert (met == 5).any() and (met == 6).any() and (met == 7).any()
    assert np.array_equal(staged, met <= KF_LDS) and staged.sum() >= 10 and (~staged).sum() >= 10
    rec = _records(d["t"], d["x"], d["y"])
    gate = (d["t"][0], d["t"][-1])
    want = O.associate(rec, d["kt"], d["circ"], gate[0], gate[1], d["max_dt"], d["tol"])
    assert 0.15 * d["n"] < len(want[1]) < 0.9 * d["n"]
    _assert_ties_taken(d["t"], d["ties"], want)
    assert (staged[d["ties"] // BLOCK]).any() and (~staged[d["ties"] // BLOCK]).any()    # ties on both paths
    _assert_same(_launch(gpu, rec, d["kt"], d["circ"], gate, d["max_dt"], d["tol"]), want)


def test_slow_stream_is_all_plain(gpu):
    """1e4 events/s against keyframes every 4 ms: a block spans 25 keyframes, every block bisects through global memory"""
    n = 20 * BLOCK
    rng = np.random.default_rng(44)
    t = T0 + np.arange(n) * 1.0e-4
    x, y = rng.integers(5, 220, n).astype(np.float64), rng.integers(5, 200, n).astype(np.float64)
    kt = np.arange(T0 + 2.0e-3, t[-1] - 0.01, 4.0e-3)         # (the last hundred events lie after the last keyframe)
    circ = _lattice(len(kt), 36)
    met, staged = _plan(t, kt)
    assert not staged.any() and met.min() > KF_LDS
    rec = _records(t, x, y)
    want = O.associate(rec, kt, circ, t[0], t[-1], 1.5e-3, 6.0)
    assert 0.15 * n < len(want[1]) < 0.9 * n
    _assert_same(_launch(gpu, rec, kt, circ, (t[0], t[-1]), 1.5e-3, 6.0), want)


# ---- 3. arbitrary order ----------------------------------------------------------------------------------------------------

def test_events_in_arbitrary_order(gpu, dense):
    """"Any order of events is taken": the stream of the threshold test permuted — every block spans the whole stream and goes
    the plain way; the oracle keeps input order, so this also pins output order = input order."""
    d = dense
    perm = np.random.default_rng(45).permutation(d["n"])
    t, x, y = d["t"][perm], d["x"][perm], d["y"][perm]
    assert not _plan(t, d["kt"])[1].any()
    rec = _records(t, x, y)
    gate = (d["t"][100], d["t"][-100])
    want = O.associate(rec, d["kt"], d["circ"], gate[0], gate[1], d["max_dt"], d["tol"])
    assert 0.15 * d["n"] < len(want[1]) < 0.9 * d["n"] and not np.all(np.diff(want[1]) > 0)
    _assert_ties_taken(d["t"], d["ties"][5:-5], want)
    _assert_same(_launch(gpu, rec, d["kt"], d["circ"], gate, d["max_dt"], d["tol"]), want)


def test_events_shuffled_inside_windows_stay_staged(gpu, sparse_kf):
    """permuted only inside windows of 4096 events: the blocks hold unsorted events and are still staged (their span meets at most
    four of the sparse keyframes)"""
    n, kf_pos = sparse_kf
    t, x, y, kt, circ, ties = _stream(n, kf_pos, 36, 46)
    rng = np.random.default_rng(47)
    perm = np.concatenate([a + rng.permutation(min(4096, n - a)) for a in range(0, n, 4096)])
    ts, xs, ys = t[perm], x[perm], y[perm]
    met, staged = _plan(ts, kt)
    assert staged.sum() >= 10 and staged.all()
    assert (np.diff(ts) < 0).sum() > n // 4
    rec = _records(ts, xs, ys)
    want = O.associate(rec, kt, circ, t[0], t[-1], 2100 * H, 6.0)
    assert 0.15 * n < len(want[1]) < 0.9 * n
    _assert_ties_taken(t, ties, want)
    _assert_same(_launch(gpu, rec, kt, circ, (t[0], t[-1]), 2100 * H, 6.0), want)


# ---- 4. exact ties and strict bounds ---------------------------------------------------------------------------------------

TIE_K = 12
TIE_H = 2.0 ** -8            # keyframe k at k * TIE_H


def _tie_events():
    """Probe events of known kinds around 12 keyframes at k * 2**-8 s, with filler events so that the time-ordered stream fills
    several blocks.  -> t, x, y, kind [n] (names), kf_time, circles, expected circle of the probes (-1: none stated)"""
    rng = np.random.default_rng(48)
    kt = np.arange(TIE_K) * TIE_H
    circ = _lattice(TIE_K, 36)
    ev = []                                                   # (t, x, y, kind, circle)
    for k in range(TIE_K):
        i = [0, 1, 2, 9, 10, 12, 17, 18, 20, 25, 26, 5][k]    # (a circle with a right-hand and a lower neighbour)
        cx, cy = circ[k, i, 0], circ[k, i, 1]
        if k + 1 < TIE_K:
            ev.append(((k + 0.5) * TIE_H,) + _tie_pixel(circ, k, i) + ("midpoint", i))      # dt to k and to k + 1 equal: k
        at = k * TIE_H                                        # exactly a keyframe time: dt = 0, the keyframe is not in question
        ev += [(at, cx, cy, "centre", i),                     # dist 0:  |0 - 6| < 6 false, < 7 true
               (at, cx + 12, cy, "equal_right", i),           # 12 px from i and from i + 1: i.  |12 - 6| < 6 false (= radius + tol), < 7 true
               (at, cx, cy + 12, "equal_below", i),           # 12 px from i and from i + 8: i
               (at, cx + 11, cy, "inside_6", i),              # one pixel inside radius + 6
               (at, cx + 5, cy + 12, "edge_7", i),            # dist exactly 13 = radius + 7: rejected by both
               (at, cx + 4, cy + 12, "inside_7", i),          # dist sqrt(160) = 12.65: inside radius + 7 only
               (at, cx + 1, cy, "near_centre", i)]
    c0, c1 = circ[0, 3], circ[TIE_K - 1, 3]
    last = (TIE_K - 1) * TIE_H
    ev += [(-TIE_H / 4, c0[0] + 3, c0[1], "before", 3), (-TIE_H, c0[0] + 3, c0[1], "before_far", 3),     # dt = max_dt exactly: rejected
           (last + TIE_H / 4, c1[0] + 3, c1[1], "after", 3), (np.nextafter(last + TIE_H / 4, 1.0), c1[0] + 3, c1[1], "after_t_max", 3),
           (float("nan"), c0[0] + 3, c0[1], "nan", -1), (float("inf"), c1[0] + 3, c1[1], "inf", -1)]
    nf = 600 * TIE_K                                           # filler: random pixels at random multiples of 2**-20 s
    ft = rng.integers(-150, int(TIE_K * TIE_H / H) + 150, nf) * H
    t = np.concatenate([[e[0] for e in ev], ft])
    x = np.concatenate([[e[1] for e in ev], rng.integers(5, 220, nf)]).astype(np.float64)
    y = np.concatenate([[e[2] for e in ev], rng.integers(5, 200, nf)]).astype(np.float64)
    kind = np.array([e[3] for e in ev] + ["filler"] * nf)
    circle = np.array([e[4] for e in ev] + [-1] * nf)
    return t, x, y, kind, kt, circ, circle


# which kinds the oracle must accept (all of them) per (max_dt, edge_tol); every other probe kind must be rejected (all of them)
_TIE_RUNS = {
    "dt_wide_tol_6": (TIE_H, 6.0, {"midpoint", "inside_6", "near_centre", "before", "after"}),
    "dt_half_tol_6": (TIE_H / 2, 6.0, {"inside_6", "near_centre", "before", "after"}),      # midpoint: dt == max_dt, strict <
    "dt_wide_tol_7": (TIE_H, 7.0, {"midpoint", "centre", "equal_right", "equal_below", "inside_6", "inside_7", "near_centre", "before", "after"}),
}


@pytest.mark.parametrize("order", ["sorted", "permuted"])
@pytest.mark.parametrize("run", sorted(_TIE_RUNS))
def test_exact_ties_and_strict_bounds(gpu, run, order):
    """Equidistant keyframes and equidistant centres go to the smaller index; dt * dt < max_dt^2 and |dist - r| < edge_tol are
    strict; t_max is inclusive; NaN and +inf times are dropped.  In time order every block is staged (the LDS form), permuted
    every block is plain: the same rules hold in both forms."""
    max_dt, tol, accepted_kinds = _TIE_RUNS[run]
    t, x, y, kind, kt, circ, circle = _tie_events()
    idx = np.argsort(t, kind="stable") if order == "sorted" else np.random.default_rng(49).permutation(len(t))
    t, x, y, kind, circle = t[idx], x[idx], y[idx], kind[idx], circle[idx]
    staged = _plan(t, kt)[1]
    assert len(staged) >= 7 and (staged.all() if order == "sorted" else not staged.any())
    gate = (-4 * TIE_H, (TIE_K - 1) * TIE_H + TIE_H / 4)
    rec = _records(t, x, y).reshape(-1, 25)
    # the oracle on the probes of each kind alone (events are judged one by one): the case is not vacuous, and the rules hold there
    for name in sorted(set(kind) - {"filler"}):
        sel = kind == name
        oo, ot, ol = O.associate(rec[sel].reshape(-1), kt, circ, gate[0], gate[1], max_dt, tol)
        if name in accepted_kinds:
            assert len(ot) == sel.sum(), name
            assert np.array_equal(ol, circle[sel].astype(np.uint32)), name      # the smaller index of the two equidistant centres
        else:
            assert len(ot) == 0, name
    want = O.associate(rec.reshape(-1), kt, circ, gate[0], gate[1], max_dt, tol)
    assert 0.2 * len(t) < len(want[1]) < 0.9 * len(t)
    _assert_same(_launch(gpu, rec.reshape(-1), kt, circ, gate, max_dt, tol), want)


# ---- 5. the block scan's carry between rounds of 1024 blocks ---------------------------------------------------------------

@pytest.mark.parametrize("n", [1024 * 1024 + 1, 2 * 1024 * 1024 + 1500])
def test_scan_carries_between_rounds(gpu, n):
    """more than 1024 blocks: scan_blocks_kernel adds the running total of the earlier rounds (1025 blocks, the last one holding one
    event; 2050 blocks = three rounds).  16 keyframes keep the brute-force oracle cheap."""
    rng = np.random.default_rng(50)
    t = T0 + np.arange(n) * H
    x, y = rng.integers(8, 202, n).astype(np.float64), rng.integers(8, 108, n).astype(np.float64)   # (~60 % within 1 .. 11 px of a centre)
    x[-1], y[-1] = 23.0, 20.0                                  # (the last event — alone in its block for 2^20 + 1 — is accepted)
    kt = T0 + (30000.5 + (n // 16) * np.arange(16.0)) * H
    circ = _lattice(16, 36)
    assert _plan(t, kt)[1].all()
    rec = _records(t, x, y)
    want = O.associate(rec, kt, circ, t[0], t[-1], 1.0, 5.0)
    first = int((want[1] < t[BLOCK * 1024]).sum())             # accepted in the first round's blocks / in the rest
    assert 0.5 * n < len(want[1]) < 0.75 * n and first > 0 and len(want[1]) - first > 0 and want[1][-1] == t[-1]
    _assert_same(_launch(gpu, rec, kt, circ, (t[0], t[-1]), 1.0, 5.0), want)


# ---- 6. sizes below and around one block ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 3, 1023, 1024, 1025])
def test_small_sizes(gpu, n):
    """a stale count word must be overwritten (with 0 for n = 0) and nothing written behind the records (_launch checks both)"""
    t, x, y, kt, circ, _ = _stream(1025, 300.0 + 400.0 * np.arange(3), 36, 51)
    x[:3], y[:3] = circ[0, 0, 0] + 3, circ[0, 0, 1]             # (the first three events are accepted)
    rec = _records(t[:n], x[:n], y[:n])
    want = O.associate(rec, kt, circ, T0, T0 + 1.0, 350 * H, 6.0)
    assert len(want[1]) >= min(n, 3) and (n < 100 or len(want[1]) < n)
    _assert_same(_launch(gpu, rec, kt, circ, (T0, T0 + 1.0), 350 * H, 6.0), want)


# ---- 7. the keyframe count the 64-ary wave search sees -------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 4096, 4097])
def test_keyframe_count(gpu, K):
    """wave_lower_bound (block_utils.hpp) at K = 1, at the sizes where its step rounds (64 | 65, 4096 | 4097) and with a second and
    third round: 8192 events against up to ten keyframes 700 events apart inside the stream, the rest of the table 3 events apart
    before the stream, after it, or half and half — so the blocks are staged and the answer of the search lies at the start, the
    middle and the end of the table.  The same events permuted take the per-thread bisection through the same tables."""
    n = 8192
    n_in = min(K, 10)
    inside = 350.0 + 700.0 * np.arange(n_in)
    for before in sorted({0, (K - n_in) // 2, K - n_in}):
        after = K - n_in - before
        kf_pos = np.concatenate([-3.0 * np.arange(before, 0, -1), inside, n + 3.0 * np.arange(1, after + 1)])
        assert len(kf_pos) == K
        t, x, y, kt, circ, ties = _stream(n, kf_pos, 4, 52)
        gate, max_dt = (t[0], t[-1]), 351 * H
        for order in ("sorted", "permuted"):
            idx = np.arange(n) if order == "sorted" else np.random.default_rng(53).permutation(n)
            staged = _plan(t[idx], kt, 4)[1]
            assert staged.all() if order == "sorted" or K <= KF_LDS else not staged.any()
            rec = _records(t[idx], x[idx], y[idx])
            want = O.associate(rec, kt, circ, gate[0], gate[1], max_dt, 6.0)
            # accepted and rejected both occur; events before the first keyframe / after the last one are among the accepted
            assert 0 < len(want[1]) < n
            assert before > 0 or (want[1] < kt[0]).any()
            assert after > 0 or (want[1] > kt[-1]).any()
            if K > 1:
                assert len(ties) >= 1 and np.isin(t[ties], want[1]).all()
            _assert_same(_launch(gpu, rec, kt, circ, gate, max_dt, 6.0), want)


# ---- 8. range tables in LDS and beyond ------------------------------------------------------------------------------------

def _range_table():
    """200 ascending, disjoint ranges over 20 blocks of events: range r = [100 r + 10, 100 r + 60] events, both ends on an event (ends
    are inclusive), gaps of 49 events between them, events before the first and after the last; range 5 is one instant holding one
    event, range 7 one instant between two events."""
    r = np.arange(200.0)
    tab = np.stack([100 * r + 10, 100 * r + 60], axis=1)
    tab[5] = (540.0, 540.0)
    tab[7] = (740.5, 740.5)
    return T0 + tab * H


@pytest.fixture(scope="module")
def ranged(gpu):
    n = 20 * BLOCK
    t, x, y, kt, circ, ties = _stream(n, _dense_kf(n), 36, 54)
    table = _range_table()
    assert table[-1, 1] < t[-1] and table[0, 0] > t[0]
    # the events on a range's start and end, and their neighbours just outside, pass the keyframe and circle gates (3 px from
    # centre 0 of their nearest keyframe): whether they come out is decided by the range alone
    for e in np.concatenate([np.rint((table.ravel() - T0) / H).astype(np.int64) + d for d in (-1, 0, 1)]):
        k = int(np.argmin(np.abs(kt - t[e])))
        x[e], y[e] = circ[k, 0, 0] + 3.0, circ[k, 0, 1]
    rec = _records(t, x, y)
    staged = _plan(t, kt)[1]
    assert staged.sum() >= 3 and (~staged).sum() >= 3          # ranges meet both forms of the keyframe search
    out = {}
    for R in (1, RNG_LDS, RNG_LDS + 1, 200):
        parts = [O.associate(rec, kt, circ, a, b, 140 * H, 6.0) for a, b in table[:R]]
        want = tuple(np.concatenate([p[j] for p in parts]) for j in range(3))
        seg = np.concatenate([np.full(len(p[1]), r, np.uint32) for r, p in enumerate(parts)])
        out[R] = (_launch(gpu, rec, kt, circ, table[:R], 140 * H, 6.0), want, seg, parts)
    return t, out


@pytest.mark.parametrize("R", [1, RNG_LDS, RNG_LDS + 1, 200])
def test_range_tables(ranged, R):
    """n_ranges <= AS_RNG_LDS = 32 is searched in LDS, 33 and 200 bisect the global table: records and segment ids equal the oracle's,
    range by range"""
    t, out = ranged
    got, want, seg, parts = out[R]
    _assert_same(got, want, seg)
    table = _range_table()[:R]
    for r in sorted({0, R - 1, min(R - 1, RNG_LDS - 1)}):                          # events exactly on a range's start and end are in
        assert parts[r][1][0] == table[r, 0] and parts[r][1][-1] == table[r, 1] and 2 < len(parts[r][1]) < 51
    # their neighbours just outside would have passed the gates (the fixture's pixels) and are not: before the first range,
    # after the last, in the gaps
    assert want[1].min() == table[0, 0] and want[1].max() == table[-1, 1]
    if R > 7:
        assert len(parts[5][1]) == 1 and parts[5][1][0] == T0 + 540 * H and len(parts[7][1]) == 0
        in_gap = (want[1][:, None] > table[None, :-1, 1]) & (want[1][:, None] < table[None, 1:, 0])
        assert not in_gap.any()


def test_longer_range_tables_agree_on_their_common_ranges(ranged):
    """the first 32 ranges are the same in the tables of 32, 33 and 200: the same records come out for them"""
    t, out = ranged
    base = out[RNG_LDS][0]
    for R in (RNG_LDS + 1, 200):
        got = out[R][0]
        keep = got["seg"] < RNG_LDS
        assert keep.sum() == base["m"] and (~keep).sum() > 0
        assert np.array_equal(_bits(got["obs"][keep]), _bits(base["obs"])) and np.array_equal(_bits(got["time"][keep]), _bits(base["time"]))
        assert np.array_equal(got["lm"][keep], base["lm"]) and np.array_equal(got["seg"][keep], base["seg"])


# ---- 9. the host form ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host(gpu):
    ctx, torch = gpu
    L = ctx._L
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    n = 5000
    t, x, y, kt, circ, ties = _stream(n, 130.5 + 227.0 * np.arange(23), 36, 55)
    rec = _records(t, x, y)
    h = vp()
    assert L.ecal_stream_create(ctx._h, rec.ctypes.data, n, ctypes.byref(h)) == ECAL_OK

    def call(kt_, circ_, K, capacity):
        obs, tm, lm = np.full((n, 2), F_SENT), np.full(n, F_SENT), np.full(n, 0xABCDEF01, np.uint32)
        count = u64(0xDEADBEEF)
        kt_ = np.ascontiguousarray(kt_, np.float64)
        rc = L.ecal_associate(ctx._h, h, kt_.ctypes.data, circ_.ctypes.data, K, 36, t[0], t[-1], 120 * H, 6.0, capacity,
                              obs.ctypes.data, tm.ctypes.data, lm.ctypes.data, ctypes.byref(count))
        return rc, int(count.value), obs, tm, lm

    yield dict(ctx=ctx, L=L, h=h, call=call, t=t, kt=kt, circ=circ, want=O.associate(rec, kt, circ, t[0], t[-1], 120 * H, 6.0))
    L.ecal_stream_destroy(h)


def test_host_form_uploads_counts_and_downloads(host):
    want = host["want"]
    m = len(want[1])
    assert 1000 < m < 5000
    for capacity in (m, 5000):
        rc, count, obs, tm, lm = host["call"](host["kt"], host["circ"], len(host["kt"]), capacity)
        assert rc == ECAL_OK and count == m
        assert np.array_equal(_bits(obs[:m]), _bits(want[0])) and np.array_equal(_bits(tm[:m]), _bits(want[1])) and np.array_equal(lm[:m], want[2])
        assert (obs[m:] == F_SENT).all() and (tm[m:] == F_SENT).all() and (lm[m:] == 0xABCDEF01).all()


def test_host_form_reports_a_short_capacity(host):
    m = len(host["want"][1])
    rc, count, obs, tm, lm = host["call"](host["kt"], host["circ"], len(host["kt"]), m - 1)
    assert rc == ECAL_ERR_RANGE and count == m
    assert (obs == F_SENT).all() and (tm == F_SENT).all() and (lm == 0xABCDEF01).all()


def test_host_form_without_keyframes(host):
    rc, count, obs, tm, lm = host["call"](host["kt"], host["circ"], 0, 5000)
    assert rc == ECAL_OK and count == 0 and (tm == F_SENT).all()


@pytest.mark.parametrize("times, bad", [([1.0, 1.0, 5.0], 1), ([T0, T0 + 2.0, T0 + 1.0], 2), ([T0, float("nan"), T0 + 1.0], 1),
                                        ([float("nan")], 0)])
def test_host_forms_refuse_keyframe_times_that_are_not_strictly_ascending(host, times, bad):
    """The keyframe search compares the first keyframe not before the event with its predecessor only, so "ties go to the smaller
    index" needs strictly ascending times ([1, 1, 5], t = 2: the kernel answers 1, the rule 0).  The entry points that have the
    table on the host refuse it and name the keyframe."""
    from eventcalib_amd import capi
    ctx, L = host["ctx"], host["L"]
    rc, count, obs, tm, lm = host["call"](times, host["circ"], len(times), 5000)
    assert rc == ECAL_ERR_INVALID and count == 0 and (tm == F_SENT).all()
    msg = L.ecal_last_error(ctx._h).decode()
    assert "ecal_associate" in msg and "strictly ascending" in msg and "keyframe %d)" % bad in msg
    # ecal_solver_create_from_stream checks the same table, after its ranges
    vp = ctypes.c_void_p
    layout = capi._SplineProblem(n_segments=1)
    kt = np.array(times, np.float64)
    ranges = np.array([host["t"][0], host["t"][-1]])
    out = vp(1)
    rc = L.ecal_solver_create_from_stream(ctx._h, host["h"], kt.ctypes.data, host["circ"].ctypes.data, len(kt), 36, ranges.ctypes.data, 1,
                                          120 * H, 6.0, ctypes.byref(layout), ctypes.byref(out))
    assert rc == ECAL_ERR_INVALID and not out.value
    msg = L.ecal_last_error(ctx._h).decode()
    assert "ecal_solver_create_from_stream" in msg and "strictly ascending" in msg and "keyframe %d)" % bad in msg
