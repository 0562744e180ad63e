"""GPU parity of the pixel DBSCAN kernel's rank table (dbscan_pixel.hpp: one u16 start per row and group of four bitmap
words; the words of the group in front of a point's own are counted when its rank is looked up): labels and cluster counts
equal to the oracle's on small segments built to sit on what that table can get wrong.  Integer pixels, eps 4.0 (integral:
the exactly-eps look-ups of phase D run) and minpts 2 unless a test says otherwise.  The second half of the file does the same on
boxes wider than the 346-column sensor (rows of up to 64 words and 16 groups) and at the kernel's admission limits."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
W, H = 346, 260


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


def _batch(segs):
    xy = np.concatenate(segs).astype(np.float64)
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint32)
    return xy, off


def _check(ctx, segs, eps=4.0, minpts=2):
    xy, off = _batch(segs)
    labels, ncl = ctx.dbscan_batch(xy, off, eps, minpts)
    ref_l, ref_n = O.dbscan_batch(xy, off[:-1], np.diff(off).astype(np.uint32), eps, minpts)
    bad = np.nonzero(labels != ref_l)[0]
    assert bad.size == 0, "%d/%d labels differ (first at %d: got %d want %d)" % (
        bad.size, labels.size, bad[0], labels[bad[0]], ref_l[bad[0]])
    assert (ncl == ref_n).all()
    return labels, ncl


def _shuffled(rng, pts):
    pts = np.unique(np.asarray(pts, np.int64), axis=0)
    return pts[rng.permutation(len(pts))]


def test_populated_rows_across_the_sensor(ctx):
    """Rows 0 .. 4 with a point every 3 pixels from x = 0 to 345: every word and every group of a row holds points, so a
    neighbour's rank that misses the words in front of it (or counts one too many) points at another pixel's entry."""
    rng = np.random.default_rng(11)
    xs = np.arange(0, W, 3)
    rows = [np.stack([xs, np.full_like(xs, y)], 1) for y in range(5)]
    one_row = _shuffled(rng, rows[0])
    five = _shuffled(rng, np.concatenate(rows))
    assert len(five) == 5 * 116
    _check(ctx, [one_row, five])


def _boundary_segments(rng):
    """An anchor point at x = a (a = 0 .. 3) fixes the bitmap's origin; patches around x = 28, 60, 124 and 252 then straddle
    the columns where the bitmap coordinate x - a + floor(eps) passes a word boundary (32, 64) and a group boundary (128, 256)."""
    segs = []
    for a in range(4):
        pts = [np.array([[a, 0]])]
        for c in (28, 60, 124, 252):
            gx, gy = np.meshgrid(np.arange(c - 6, c + 7), np.arange(10, 19))
            patch = np.stack([gx.ravel(), gy.ravel()], 1)
            pts.append(patch[rng.random(len(patch)) < 0.6])
            pts.append(np.stack([np.arange(c - 8, c + 9, 4), np.full(5, 30)], 1))   # a row of exactly-eps pairs over the boundary
        segs.append(_shuffled(rng, np.concatenate(pts)))
        assert len(segs[-1]) <= 768
    return segs


@pytest.mark.parametrize("eps", [4.0, 3.0])
def test_group_and_word_boundaries(ctx, eps):
    """eps 4.0 runs the kernel with the disc compiled in, eps 3.0 the generic one; both integral."""
    _check(ctx, _boundary_segments(np.random.default_rng(12)), eps)


def test_full_segment_and_one_more(ctx):
    """768 points fill the first pass's capacity; 769 must come back from the list tier (the 2048-point layout) with the
    oracle's labels.  A 32 x 24 lattice of spacing 4: every neighbour is an exactly-eps pair, the quirk bites."""
    rng = np.random.default_rng(13)
    gx, gy = np.meshgrid(4 * np.arange(32), 4 * np.arange(24))
    lat = np.stack([gx.ravel(), gy.ravel()], 1)
    full = _shuffled(rng, lat)
    more = _shuffled(rng, np.concatenate([lat, [[2, 2]]]))
    assert len(full) == 768 and len(more) == 769
    _check(ctx, [full, more])


def test_box_shapes_at_and_past_the_table(ctx):
    """The table holds 1032 entries (rows x groups of the padded box).  The sensor's largest box, (0, 0) .. (345, 259), is
    268 rows x 3 groups = 804 and stays in the pixel kernel; the only shapes past the table are 9 words wide and 345 .. 359
    rows high, which no box inside 346 x 260 is — so this one segment leaves the sensor: the same two corners turned by 90
    degrees, (0, 0) .. (259, 345), 354 rows x 3 groups = 1062.  It goes to the to-do list and the general tiers label it
    (test_gpu_dbscan.py::test_size_tiers_and_big_path tells the tiers apart by nothing but their labels either)."""
    rng = np.random.default_rng(14)
    t = np.arange(0, 260)
    diag = np.stack([(t * 345) // 259, t], 1)
    inside = _shuffled(rng, np.concatenate([[[0, 0], [345, 259]], diag, np.clip(diag + [[3, 0]], 0, [W - 1, H - 1])]))
    turned = inside[:, ::-1].copy()
    assert turned[:, 1].max() == 345 and turned[:, 0].max() == 259
    for eps in (4.0, 3.0):
        _check(ctx, [inside, turned, inside], eps)


def test_dense_rows(ctx):
    """More than 255 points in one row (the table's entries are u16: no per-row limit is left): 300 in one row, all 346
    pixels of another, and a few rows around them."""
    rng = np.random.default_rng(15)
    a = np.stack([np.arange(300), np.full(300, 7)], 1)
    b = np.stack([np.arange(W), np.full(W, 12)], 1)
    c = np.stack([rng.integers(0, W, 100), rng.integers(5, 16, 100)], 1)
    seg = _shuffled(rng, np.concatenate([a, b, c]))
    assert 646 <= len(seg) <= 768
    only_row = _shuffled(rng, np.stack([np.arange(256), np.full(256, 3)], 1))
    _check(ctx, [seg, only_row])


def test_list_tier_layout_over_the_full_sensor(ctx):
    """1500 points (the 2048-point layout of the list kernel) spread over the whole sensor: a thinned lattice of spacing 4
    (exactly-eps pairs) and uniform pixels on top."""
    rng = np.random.default_rng(16)
    gx, gy = np.meshgrid(np.arange(1, W, 4), np.arange(1, H, 4))
    lat = np.stack([gx.ravel(), gy.ravel()], 1)
    lat = lat[rng.random(len(lat)) < 0.2]
    uni = np.stack([rng.integers(0, W, 3000), rng.integers(0, H, 3000)], 1)
    pts = _shuffled(rng, np.concatenate([lat, uni, [[0, 0], [W - 1, H - 1]]]))
    corners = np.array([[0, 0], [W - 1, H - 1]])
    seg = np.concatenate([corners, pts[:1498]])
    seg = _shuffled(rng, seg)
    assert 1490 <= len(seg) <= 1500
    _check(ctx, [seg])
    _check(ctx, [seg], 3.0)


# ---- boxes wider than 346 columns: rows of up to 64 words and 16 groups (the first pass's 11-bit bitmap coordinates), up to 32
# words for the second pass (10 bits).  Which kernel labelled a segment is read from the passes' to-do counters
# (Context.debug_px_todo_counts): a segment the pixel kernel kept is on no list.

def _general(ctx, xy, off, eps, minpts):
    """The same batch through the general tiers alone (ECAL_FORCE=dbscan_general)."""
    import os
    from eventcalib_amd import capi
    os.environ["ECAL_FORCE"] = "dbscan_general"
    capi.sync_env()
    try:
        return ctx.dbscan_batch(xy, off, eps, minpts)
    finally:
        os.environ.pop("ECAL_FORCE", None)
        capi.sync_env()


def _check_both(ctx, segs, eps=4.0, minpts=2):
    """Labels == the oracle's and == the general tiers'; returns what the pixel passes listed: (first, second or None)."""
    labels, ncl = _check(ctx, segs, eps, minpts)
    listed = ctx.debug_px_todo_counts()
    xy, off = _batch(segs)
    gl, gn = _general(ctx, xy, off, eps, minpts)
    assert np.array_equal(labels, gl) and np.array_equal(ncl, gn)
    return listed


def _rows(rng, width, sp, nrows, npts):
    """Row 0 with a point every sp pixels from x = 0 to below `width`: every word and every group of the row holds points.  Rows
    1 .. nrows - 1 hold the same columns, thinned until the segment has npts points.  The callers' sp and nrows are such that no two
    points are exactly eps apart along an axis (eps 4.0: every 3 px, rows 0 .. 3; eps 3.0: every 4 or 2 px, rows 0 .. 2): the pruning
    quirk makes no one-way edge (more than 64 of them hand a segment to the general tiers), nothing but the box decides the tier."""
    xs = np.arange(0, width, sp)
    row0 = np.stack([xs, np.zeros_like(xs)], 1)
    gx, gy = np.meshgrid(xs, np.arange(1, nrows))
    rest = np.stack([gx.ravel(), gy.ravel()], 1)
    assert len(row0) <= npts <= len(row0) + len(rest)
    return _shuffled(rng, np.concatenate([row0, rest[rng.permutation(len(rest))][: npts - len(row0)]]))


def _words(seg, eps):
    return (int(seg[:, 0].max() - seg[:, 0].min()) + 1 + 2 * int(eps) + 31) // 32


@pytest.mark.parametrize("eps", [4.0, 3.0])
def test_populated_rows_across_wider_sensors(ctx, eps):
    """First pass (<= 768 points): rows across 640, 1280 and 2039 columns = 21, 41 and 64 words, 6, 11 and 16 groups (2039 + 2 floor(eps)
    <= 2047 is the widest box its coordinates hold).  Second pass (769 .. 2048 points, box <= 1023 columns): 640 and 1015 columns,
    21 and 32 words."""
    rng = np.random.default_rng(21)
    sp, nrows = (3, 4) if eps == 4.0 else (4, 3)
    first = [_rows(rng, w, sp, nrows, n) for w, n in ((640, 450), (1280, 768), (2039, 768))]
    assert [_words(s, eps) for s in first] == [21, 41, 64]
    assert _check_both(ctx, first, eps) == (0, None)
    sp, nrows = (3, 4) if eps == 4.0 else (2, 3)
    second = [_rows(rng, w, sp, nrows, n) for w, n in ((640, 769), (1015, 900), (1015, 1300))]
    assert [_words(s, eps) for s in second] == [21, 32, 32]
    assert _check_both(ctx, second, eps) == (3, 0)


def _wide_boundary_segments(rng, eps):
    """_boundary_segments on wide rows: an anchor at x = a (a = 0 .. 3) fixes the bitmap's origin; around every column c whose bitmap
    coordinate c - a + floor(eps) is 32 k or 128 k, k = 1 .. 15 (words 1 .. 60, groups 1 .. 15), a patch that straddles it and a row
    of exactly-eps pairs over it; seven boundaries to a segment.  The patches' columns and rows leave no two of their points exactly
    eps apart along an axis, so a segment has at most 7 x 4 one-way edges (the rows') and stays in the pixel kernel."""
    rd = int(eps)
    offs, nrows = ([-10, -9, -8, -7, -2, -1, 0, 1, 6, 7, 8, 9], 4) if rd == 4 else ([-7, -6, -5, -1, 0, 1, 5, 6, 7], 3)
    assert not any(abs(p - q) == rd for p in offs for q in offs)
    bounds = sorted(set(32 * k for k in range(1, 16)) | set(128 * k for k in range(1, 16)))
    segs = []
    for a in range(4):
        for lo in range(0, len(bounds), 7):
            pts = [np.array([[a, 0]])]
            for b in bounds[lo:lo + 7]:
                c = b - rd + a                      # bitmap column b: the first bit of a word (of a group)
                gx, gy = np.meshgrid(c + np.array(offs), np.arange(10, 10 + nrows))
                patch = np.stack([gx.ravel(), gy.ravel()], 1)
                pts.append(patch[rng.random(len(patch)) < 0.6])
                pts.append(np.stack([np.arange(c - 2 * rd, c + 2 * rd + 1, rd), np.full(5, 30)], 1))   # exactly-eps pairs over the boundary
            segs.append(_shuffled(rng, np.concatenate(pts)))
            assert len(segs[-1]) <= 768
    return segs


@pytest.mark.parametrize("eps", [4.0, 3.0])
def test_group_and_word_boundaries_beyond_256(ctx, eps):
    segs = _wide_boundary_segments(np.random.default_rng(22), eps)
    assert max(_words(s, eps) for s in segs) == 61
    assert _check_both(ctx, segs, eps) == (0, None)


def _box(rng, span_x, span_y, pad, npts=0):
    """A segment whose bounding box is span_x x span_y pixels — padded by the disc on both sides, W = span_x + pad columns and
    H = span_y + pad rows of bitmap — made of pairs of neighbouring pixels (x, y), (x + 1, y) whose x and y are multiples of 7:
    clusters of two, and no two points exactly eps (3 or 4) apart along an axis, so that no one-way edge and nothing else but
    the box decides whether the pixel kernel keeps it.  One pair in each corner, the others on the diagonal (npts = 0) or
    drawn from the whole lattice until the segment holds npts points."""
    corner = [[0, 0], [1, 0], [span_x - 1, span_y - 1], [span_x - 2, span_y - 1]]
    nx, ny = (span_x - 12) // 7, (span_y - 12) // 7
    if npts:
        gx, gy = np.meshgrid(7 * np.arange(1, nx + 1), 7 * np.arange(1, ny + 1))
        c = np.stack([gx.ravel(), gy.ravel()], 1)
        c = c[rng.permutation(len(c))][: (npts - 4) // 2]
    else:
        m = max(nx, ny)
        i = np.arange(1, m + 1)
        c = np.unique(np.stack([7 * np.maximum(1, i * nx // m), 7 * np.maximum(1, i * ny // m)], 1), axis=0)[:300]
    seg = _shuffled(rng, np.concatenate([corner, c, c + [[1, 0]]]))
    assert seg[:, 0].min() == 0 and seg[:, 1].min() == 0 and seg[:, 0].max() == span_x - 1 and seg[:, 1].max() == span_y - 1
    return seg


# (name, padded W, padded H inside, padded H outside): the conditions of px_segment, dbscan_pixel.hpp — H <= 472 rows,
# H * ceil(W / 32) <= 3232 words, H * ceil(ceil(W / 32) / 4) <= 1032 rank entries
_LIMITS = [("21 words x 153 | 154 rows", 648, 153, 154), ("41 words x 78 | 79 rows", 1288, 78, 79), ("64 words x 50 | 51 rows", 2047, 50, 51),
           ("9 words, 3 groups x 344 | 345 rows", 288, 344, 345), ("472 | 473 rows", 28, 472, 473)]


@pytest.mark.parametrize("eps", [4.0, 3.0])
@pytest.mark.parametrize("name,W,H_in,H_out", _LIMITS, ids=[x[0].replace(" ", "_").replace("|", "or") for x in _LIMITS])
def test_admission_limits(ctx, eps, name, W, H_in, H_out):
    """One segment just inside and one just outside each limit of the pixel kernel's bitmap and rank table: both labelled as the
    oracle labels them, the first by the pixel kernel (on no list), the second by the general tiers (listed)."""
    pad = 2 * int(eps)
    rw = (W + 31) // 32
    ng = (rw + 3) // 4
    assert H_in <= 472 and H_in * rw <= 3232 and H_in * ng <= 1032 and W <= 2047
    assert H_out > 472 or H_out * rw > 3232 or H_out * ng > 1032
    rng = np.random.default_rng(23)
    inside, outside = _box(rng, W - pad, H_in - pad, pad), _box(rng, W - pad, H_out - pad, pad)
    assert len(inside) <= 768 and len(outside) <= 768
    assert _check_both(ctx, [inside], eps) == (0, None)
    assert _check_both(ctx, [outside], eps) == (1, None)
    assert _check_both(ctx, [inside, outside, inside], eps) == (1, None)


@pytest.mark.parametrize("eps", [4.0, 3.0])
def test_admission_by_coordinate_bits(ctx, eps):
    """W <= CMASK: a padded box 2047 columns wide is the first pass's (11-bit bitmap coordinates), 2048 is not; on segments of
    769 .. 2048 points, the second pass's (10 bits), 1023 is and 1024 is not — the first pass lists those for their size alone."""
    pad = 2 * int(eps)
    rng = np.random.default_rng(24)
    assert _check_both(ctx, [_box(rng, 2047 - pad, 20, pad)], eps) == (0, None)
    assert _check_both(ctx, [_box(rng, 2048 - pad, 20, pad)], eps) == (1, None)
    inside, outside = _box(rng, 1023 - pad, 70, pad, 900), _box(rng, 1024 - pad, 70, pad, 900)
    assert len(inside) == 900 and len(outside) == 900
    assert _check_both(ctx, [inside], eps) == (1, 0)
    assert _check_both(ctx, [outside], eps) == (1, 1)
    full = _box(rng, 1023 - pad, 101 - pad, pad, 2048)             # the second pass's capacity on its widest rows: 32 words x 101 rows = 3232
    assert len(full) == 2048
    assert _check_both(ctx, [full], eps) == (1, 0)
    tall = _box(rng, 200, 473 - pad, pad, 900)                       # the second pass's rows: H <= 472 as in the first
    assert _check_both(ctx, [tall, inside], eps) == (2, 1)
