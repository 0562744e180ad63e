"""Hand-built windows for the fitCircle == 1 pairing (CirclesEventFrame.cpp:180-281) — test infrastructure.

A window is a list of integer pixels per polarity: rasterised rings split into a + arc and a - arc, rows, diagonals, blocks,
single pixels, any of them given twice.  build() packs the windows as event records (synth_stream.pack_records), one time window
each, so that they travel the normal path: records -> slicer -> DBSCAN -> extraction.  Everything is on integer pixels, so
squared distances, the nine sums of the circle fit and every equality a scene is built around are exact.

pairing_trace() restates the pairing itself in numpy scalars — neighbour list sorted by (squared distance, cluster index), cut at
the number of kept clusters, the two gates, the algebraic fit, first minimum, noise test, back-check — on the kept clusters and
representatives of an oracle result, and says per + cluster which rule ended it.  The tests use it to show that a scene
reaches the rule it was built for, and as a second statement of the pairing next to oracle/detect_oracle.cpp.
"""
import math

import numpy as np
import torch

import synth_stream as SS

POS, NEG = 1, 0          # Event polarity byte of the + and of the - pixel set
WINDOW = 1.5e-3
T_START = 5.0


# ---- shapes: lists of (x, y) integer pixels ----
def ring(cx, cy, r, axis=(1, 0)):
    """Rasterised circle (pixels within half a pixel of the radius) split by the line through the centre normal to `axis`:
    returns (+ arc, - arc); pixels on the line itself are left out."""
    pos, neg = [], []
    for x in range(cx - r - 1, cx + r + 2):
        for y in range(cy - r - 1, cy + r + 2):
            if abs(math.hypot(x - cx, y - cy) - r) < 0.5:
                s = (x - cx) * axis[0] + (y - cy) * axis[1]
                if s > 0:
                    pos.append((x, y))
                elif s < 0:
                    neg.append((x, y))
    return pos, neg


def row(x0, y, n):
    return [(x0 + i, y) for i in range(n)]


def diagonal(x0, y0, n):
    return [(x0 + i, y0 + i) for i in range(n)]


def block(x0, y0, w, h):
    return [(x0 + i, y0 + j) for j in range(h) for i in range(w)]


def pixel(x, y):
    return [(x, y)]


def shifted(pts, dx, dy):
    return [(x + dx, y + dy) for x, y in pts]


def median_rep(pts):
    """The representative of a cluster of these pixels (:136-147): the member of rank size / 2 by norm.  Raises when another
    member has that norm (the pick then depends on the member order) — the scenes are built without such ties."""
    a = np.array(sorted(set(pts)), np.int64)
    key = (a ** 2).sum(1)
    o = np.argsort(key, kind="stable")
    m = o[len(a) // 2]
    if (key == key[m]).sum() != 1:
        raise ValueError("tied median")
    return int(a[m, 0]), int(a[m, 1])


def place(pts, rep_at):
    """`pts` translated so that the translated cluster's representative is exactly the pixel rep_at (tried member by member:
    the representative depends on where the cluster lies)."""
    for m in sorted(set(pts)):
        cand = shifted(pts, rep_at[0] - m[0], rep_at[1] - m[1])
        if min(min(p) for p in cand) < 0:
            continue
        try:
            if median_rep(cand) == tuple(rep_at):
                return cand
        except ValueError:
            pass
    raise ValueError("no translation puts the representative at %r" % (rep_at,))


def board(rows, cols, x0=20, y0=20, pitch_x=30, pitch_y=24, r=8):
    """rows x cols rings; returns (+ pixels, - pixels, centres)."""
    pos, neg, centres = [], [], []
    for i in range(rows):
        for j in range(cols):
            c = (x0 + pitch_x * j, y0 + pitch_y * i)
            p, n = ring(c[0], c[1], r)
            pos += p
            neg += n
            centres.append(c)
    return pos, neg, centres


def scattered(n, x0, y0, width, pitch=6, shape=((0, 0),)):
    """n copies of `shape` on a lattice of the given pitch, `width` copies per lattice row, from (x0, y0): with a pitch beyond
    the DBSCAN radius plus the shape's extent the copies never touch — single pixels stay noise, small shapes stay clusters
    of their own."""
    out = []
    for k in range(n):
        ox, oy = x0 + pitch * (k % width), y0 + pitch * (k // width)
        out += [(ox + sx, oy + sy) for sx, sy in shape]
    return out


# ---- windows -> records ----
class Window:
    def __init__(self, pos=(), neg=()):
        self.pos, self.neg = list(pos), list(neg)

    def add(self, pos=(), neg=()):
        self.pos += list(pos)
        self.neg += list(neg)
        return self

    def points(self):
        """The window's unique pixels per polarity (float64 [n, 2] each, sorted)."""
        return tuple(np.array(sorted(set(p)), np.float64).reshape(-1, 2) for p in (self.pos, self.neg))


def build(windows, seed=0, length=WINDOW, t_start=T_START):
    """Packs the windows (events shuffled inside each, duplicates kept) -> dict(buf: uint8 tensor of records, t0, t1: the
    inclusive time windows, points: per window (+ pixels, - pixels), n: events)."""
    rng = np.random.default_rng(seed)
    ts, xs, ps = [], [], []
    for s, w in enumerate(windows):
        ev = [(x, y, POS) for x, y in w.pos] + [(x, y, NEG) for x, y in w.neg]
        assert ev, "an empty window"
        ev = [ev[i] for i in rng.permutation(len(ev))]
        ts.append(t_start + s * length + np.sort(rng.uniform(0.0, 0.98 * length, len(ev))))
        xs.append(np.array([(e[0], e[1]) for e in ev], np.float64))
        ps.append(np.array([e[2] for e in ev], np.uint8))
    S = len(windows)
    buf = SS.pack_records(torch.tensor(np.concatenate(ts)), torch.tensor(np.concatenate(xs)), torch.tensor(np.concatenate(ps)))
    t0 = t_start + length * np.arange(S)
    t1 = np.nextafter(t_start + length * np.arange(1, S + 1), -np.inf)
    return dict(buf=buf, t0=t0, t1=t1, points=[w.points() for w in windows], n=int(sum(len(t) for t in ts)))


# ---- the pairing, restated ----
F = np.float64
DBL_MAX = np.finfo(np.float64).max


def neighbours(q, reps, K, thr):
    """The gated neighbour list of :184-193 / :233-241 under the project's contract: the K nearest representatives sorted by
    (squared distance, cluster index), ending at the number of clusters present, then cut by d > 4 d0 and by d > 4 thr^2.
    Returns (cluster indices kept, all squared distances of the uncut list, what cut it: 'ratio' / 'gate' / None)."""
    d = ((np.asarray(reps, F) - np.asarray(q, F)) ** 2).sum(1)
    order = np.lexsort((np.arange(len(d)), d))[:K]
    dd = d[order]
    for oi in range(len(order)):
        if dd[oi] > dd[0] * 4:
            return order[:oi], dd, "ratio"
        if dd[oi] > 4 * F(thr) * F(thr):
            return order[:oi], dd, "gate"
    return order, dd, None


def fit_circle(pts):
    """fitCircle (:361-415): nine sums, 3x3 system, partial-pivot elimination, every step one IEEE operation."""
    with np.errstate(all="ignore"):
        x, y = pts[:, 0].astype(F), pts[:, 1].astype(F)
        sx, sy, sxx, syy, sxy = x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()
        sxxx, syyy, sxyy, sxxy = (x * x * x).sum(), (y * y * y).sum(), (x * y * y).sum(), (x * (x * y)).sum()
        A = [[2 * sx, 2 * sy, F(len(pts)), sxx + syy], [2 * sxx, 2 * sxy, sx, sxxx + sxyy], [2 * sxy, 2 * syy, sy, sxxy + syyy]]
        for c in range(3):
            piv = c
            for r in range(c + 1, 3):
                if abs(A[r][c]) > abs(A[piv][c]):
                    piv = r
            A[c], A[piv] = A[piv], A[c]
            for r in range(c + 1, 3):
                f = A[r][c] / A[c][c]
                for k in range(c, 4):
                    A[r][k] = A[r][k] - f * A[c][k]
        v = [F(0)] * 3
        for r in (2, 1, 0):
            t = A[r][3]
            for k in range(r + 1, 3):
                t = t - A[r][k] * v[k]
            v[r] = t / A[r][r]
        return v[0], v[1], np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2])


def fit_pair(P, N, rp, rn, thr):
    """(err, radius, cx, cy) of :202-219 for one + cluster and one - cluster (members [m, 2]) with representatives rp, rn."""
    with np.errstate(all="ignore"):
        cx, cy, r = fit_circle(np.concatenate([P, N]))
        a = F(rp[0]) - F(rn[0]), F(rp[1]) - F(rn[1])
        approx = np.sqrt(a[0] * a[0] + a[1] * a[1]) / 2
        if r > thr or r > 2 * approx:
            return DBL_MAX, r, cx, cy
        err = F(0)
        for e in np.concatenate([P, N]).astype(F):
            ex, ey = e[0] - cx, e[1] - cy
            err = err + abs(np.sqrt(ex * ex + ey * ey) - r)
        return err / (F(len(P) + len(N)) * r), r, cx, cy


def pairing_trace(pos, neg, ref, thr, K):
    """The whole of :180-281 on the kept clusters and representatives of `ref` (an oracle_lib.extract_candidates result for
    pos / neg).  Returns dict(pair [n, 2], xyr [n, 3], steps): steps[pi] = dict(fwd: gated neighbour list, fwd_d2, fwd_cut,
    fits: the forward fits, nmin, end: which rule ended the cluster — 'empty' (no neighbour survives), 'noise' (the best
    forward fit fails err < 2 / r), 'back_empty', 'back' (the back-check names another + cluster), 'ok' — and, where
    reached, back, back_d2, back_cut, back_fits, pmin)."""
    pos, neg = np.asarray(pos, F), np.asarray(neg, F)
    Pc = [pos[ref["kept_pos"] == k] for k in range(ref["nk_pos"])]
    Nc = [neg[ref["kept_neg"] == k] for k in range(ref["nk_neg"])]
    rp, rn = pos[ref["rep_pos"]], neg[ref["rep_neg"]]
    pair, xyr, steps = [], [], []

    def first_min(fits):
        m = 0
        for j in range(1, len(fits)):
            if fits[j][0] < fits[m][0]:
                m = j
        return m

    with np.errstate(all="ignore"):
        for pi in range(len(Pc)):
            st = dict(end="ok")
            steps.append(st)
            st["fwd"], st["fwd_d2"], st["fwd_cut"] = neighbours(rp[pi], rn, K, thr)
            if len(st["fwd"]) == 0:
                st["end"] = "empty"
                continue
            st["fits"] = [fit_pair(Pc[pi], Nc[j], rp[pi], rn[j], thr) for j in st["fwd"]]
            st["nmin"] = nmin = first_min(st["fits"])
            best = st["fits"][nmin]
            if not best[0] < 2 / best[1]:
                st["end"] = "noise"
                continue
            nsel = int(st["fwd"][nmin])
            st["back"], st["back_d2"], st["back_cut"] = neighbours(rn[nsel], rp, K, thr)
            if len(st["back"]) == 0:
                st["end"] = "back_empty"
                continue
            st["back_fits"] = [fit_pair(Pc[i], Nc[nsel], rp[i], rn[nsel], thr) for i in st["back"]]
            st["pmin"] = pmin = first_min(st["back_fits"])
            if int(st["back"][pmin]) != pi:
                st["end"] = "back"
                continue
            f = st["back_fits"][pmin]
            pair.append((pi, nsel))
            xyr.append((f[2], f[3], f[1]))
    return dict(pair=np.array(pair, np.uint32).reshape(-1, 2), xyr=np.array(xyr, F).reshape(-1, 3), steps=steps)


# ---- the scenes ----
THR = 15.5
T_AT = 9.0                                           # 4 * 9^2 == 324 == 18^2 exactly
T_BELOW = float(np.nextafter(np.float64(9.0), 0.0))  # the next radius threshold below it: 4 thr^2 < 324


class Group:
    """Windows that share their detection parameters: run together, as one stream."""

    def __init__(self, name, windows, names, cluster_min=5, need=1, thr=THR, knn=(3,), minpts=2):
        self.name, self.windows, self.names = name, windows, names
        self.cluster_min, self.need, self.thr, self.knn, self.minpts = cluster_min, need, thr, tuple(knn), minpts

    def build(self, seed=0):
        return build(self.windows, seed=seed)


def _ring0(shift=(0, 0)):
    p, n = ring(30, 30, 8)
    return shifted(p, *shift), shifted(n, *shift)


def knn_board():
    """3 x 4 rings, pitch 30 x 24: a + arc's nearest - representatives are its own ring's, the next ring's in its row and
    the rings' above and below; three - blocks beside the + arc of the last ring of the middle row bring its gated list
    to five."""
    p, n, c = board(3, 4)
    cx, cy = c[7]
    dec = block(cx + 21, cy - 7, 3, 2) + block(cx + 21, cy + 6, 3, 2) + block(cx + 26, cy, 3, 2)
    return Group("knn_board", [Window(p, n + dec)], ["board"], need=12, knn=range(1, 9))


def tie_group():
    """A ring (representatives 16 apart) and a - decoy, a 12-pixel-radius arc, whose representative is the mirror image of
    the ring's - representative in its + one: two neighbours at squared distance 256, one on each side.  With knn_num = 1
    the one of the smaller cluster index is the list; which of the two that is depends on where the scene lies (the
    clusters are numbered in the order of the window's pixel set): the partner in the first window, the decoy in the
    second."""
    _, big = ring(0, 0, 12)
    wins = []
    for sh in ((0, 0), (0, 5)):
        p, n = _ring0(sh)
        rp, rn = median_rep(p), median_rep(n)
        wins.append(Window(p, n + place(big, (2 * rp[0] - rn[0], 2 * rp[1] - rn[1]))))
    return Group("tie", wins, ["partner_first", "decoy_first"], knn=(1, 2))


def ratio_group():
    """The ring of ring(30, 30, 8): + representative (38, 30), - representative (22, 30), squared distance 256.  A - block
    inside the ring is the nearest neighbour: with its representative on the centre d0 = 64 and the partner sits at
    exactly 4 d0 (kept: the test is d > 4 d0); with the - arc one pixel lower, its representative on (22, 31), the
    partner is at 16^2 + 1 = 257 = 4 d0 + 1, the next squared pixel distance there is, and is cut; with the block on
    (31, 27) d0 = 58, 4 d0 = 232 < 256 and the partner is cut from further off; the last window has a - cluster whose
    representative is the pixel next to the + one (d0 = 1: everything else is cut)."""
    p, n = _ring0()
    assert median_rep(p) == (38, 30) and median_rep(n) == (22, 30)
    blk = block(0, 0, 3, 2)
    tee = [(39, y) for y in range(28, 33)] + [(40, 30), (41, 30)]
    wins = [Window(p, n + place(blk, (30, 30))), Window(p, place(n, (22, 31)) + place(blk, (30, 30))),
            Window(p, n + place(blk, (31, 27))), Window(p, n + place(tee, (39, 30)))]
    return Group("ratio", wins, ["at_4d0", "at_4d0_plus_1", "beyond_4d0", "adjacent"], knn=(2, 3))


def _tees():
    tp = [(39, 30 + y) for y in range(-2, 3)] + [(39 - k, 30) for k in range(1, 4)]
    tn = [(21, 30 + y) for y in range(-2, 3)] + [(21 + k, 30) for k in range(1, 4)]
    return place(tp, (39, 30)), place(tn, (21, 30))


def gate_groups():
    """Two T-shaped clusters, bars outside, whose representatives lie on the bars, 18 apart (squared distance 324), around
    a fitted circle of radius 8.46: with radius_threshold = 9 the neighbour is at exactly 4 thr^2 (kept: d > 4 thr^2 cuts)
    and the pair is a candidate; with the next double below 9 it is cut and the window has none."""
    tp, tn = _tees()
    return [Group("gate_at", [Window(tp, tn)], ["tees"], thr=T_AT, knn=(2,)),
            Group("gate_below", [Window(tp, tn)], ["tees"], thr=T_BELOW, knn=(2,))]


def back_group():
    """Two + arcs, radius 8 and radius 13 about one centre, and the - arc of radius 8: both take the - arc as their best
    forward fit, the back-check gives it to the inner one."""
    p, n = _ring0()
    p2, _ = ring(30, 30, 13)
    return Group("back", [Window(p + p2, n)], ["two_plus_one_minus"], knn=(3,))


def degenerate_groups():
    """Collinear pairs (the 3 x 3 system is singular: centre and radius come out inf or NaN) alone and beside good rings;
    with cluster_min = 1 and minpts = 1 the smallest clusters there are: two single pixels (no cluster at any minpts >= 1 —
    dbscan.h counts a point's neighbours without the point itself — so the window fails the cluster count) and pairs of
    two-pixel clusters, four pixels on a square (an exact circle) and four on a line."""
    p, n, _ = board(2, 2)
    five = Group("collinear", [Window(row(10, 20, 5), row(17, 20, 5)), Window(diagonal(10, 10, 5), diagonal(17, 17, 5)),
                               Window(p + row(90, 30, 5), n + row(97, 30, 5)), Window(p + row(90, 30, 5) * 2, n + row(97, 30, 5) * 3)],
                 ["row", "diagonal", "among_rings", "among_rings_duplicated"], knn=(1, 3))
    tiny = Group("tiny", [Window(pixel(10, 10), pixel(13, 10)), Window(row(10, 10, 2), row(10, 13, 2)),
                          Window(row(10, 10, 2), row(13, 10, 2))],
                 ["two_pixels", "two_pairs_square", "two_pairs_collinear"], cluster_min=1, minpts=1, knn=(1, 3))
    return [five, tiny]


def short_groups():
    """Fewer kept clusters than knn_num: 2 x 2 rings (4 and 4), 2 x 3 rings (6 and 6), and 2 x 2 rings with five more -
    blocks (4 and 9: only the + side is short)."""
    p, n, c = board(2, 2)
    p6, n6, _ = board(2, 3)
    extra = []
    for k in range(5):
        extra += block(100 + 8 * k, 20 + 9 * (k % 2), 3, 2)
    return [Group("short_2x2", [Window(p, n)], ["2x2"], need=4, knn=(5, 6, 8)),
            Group("short_2x3", [Window(p6, n6)], ["2x3"], need=6, knn=(8,)),
            Group("short_one_side", [Window(p, n + extra)], ["plus_side_short"], need=4, knn=(8,))]


def tier_group(kind):
    """The 3 x 4 board and enough lattice noise for a tier of the extraction: 'first' (the board alone), 'points' (isolated
    pixels, DBSCAN noise, beyond the first pass's point count), 'clusters' (two-pixel + clusters — clusters with minpts = 1,
    kept with cluster_min = 2 — beyond the first pass's cluster count), 'global' (isolated pixels beyond the second pass's point count)."""
    p, n, _ = board(3, 4)
    base = len(set(p)) + len(set(n))
    if kind == "first":
        return Group("tier_first", [Window(p, n)], [kind], need=12)
    if kind == "clusters":
        return Group("tier_clusters", [Window(p + scattered(390, 3, 100, 48, 7, ((0, 0), (1, 0))), n)], [kind], cluster_min=2, need=12,
                     minpts=1)
    # 40 points beyond DET_LDS_PTS (1408) and beyond DET_LDS_PTS2 (2816) of extract_window.hpp; the GPU test asserts the
    # sizes it reads back against the header's own values, so a changed threshold fails there
    total = {"points": 1408 + 40, "global": 2816 + 40}[kind]
    sites = scattered(total - base, 2, 95, 68, 5)
    return Group("tier_" + kind, [Window(p + sites[0::2], n + sites[1::2])], [kind], need=12)


def all_groups():
    return ([knn_board(), tie_group(), ratio_group()] + gate_groups() + [back_group()] + degenerate_groups() + short_groups()
            + [tier_group(k) for k in ("first", "points", "clusters", "global")])


def oracle_windows(group, K, oracle):
    """The group's windows through the oracle alone: records -> window bounds -> EventFrame in the reference's order ->
    extraction with fitCircle and knn_num = K.  Returns a list of (pos, neg, result, trace or None)."""
    b = group.build()
    rec = b["buf"].numpy()
    out = []
    for s in range(len(group.windows)):
        lo, hi = oracle.window_bounds(rec, b["t0"][s], b["t1"][s])
        pos, neg, _ = oracle.event_frame(rec, lo, hi, "reference")
        assert {tuple(q) for q in pos} == {tuple(q) for q in b["points"][s][0]} and {tuple(q) for q in neg} == {tuple(q) for q in b["points"][s][1]}
        ref = extract(oracle, pos, neg, group, K)
        out.append((pos, neg, ref, None if ref["status"] else pairing_trace(pos, neg, ref, group.thr, K)))
    return out


def extract(oracle, pos, neg, group, K, override_pos=None, override_neg=None):
    return oracle.extract_candidates(pos, neg, 4.0, group.minpts, group.cluster_min, group.need, group.thr, True, K, override_pos, override_neg)


def coincident_points():
    """(+ pixels, - pixels) of the ring of ratio_group() and a - block whose representative IS the + representative's pixel
    (38, 30): d0 = 0.  No event window holds this — a pixel of both polarities is erased from both sets (EventFrame.cpp:24-32)
    — so the two point sets go to the DBSCAN and extraction stages directly."""
    p, n = _ring0()
    pos, neg = Window(p, n + place(block(0, 0, 3, 2), (38, 30))).points()
    assert (38.0, 30.0) in {tuple(q) for q in pos} and (38.0, 30.0) in {tuple(q) for q in neg}
    return pos, neg
