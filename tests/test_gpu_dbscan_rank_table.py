"""GPU parity of the pixel DBSCAN kernel's rank table (dbscan_pixel.hpp: one u16 start per row and group of four bitmap
words; the words of the group in front of a point's own are counted when its rank is looked up): labels and cluster counts
equal to the oracle's on small segments built to sit on what that table can get wrong.  Integer pixels, eps 4.0 (integral:
the exactly-eps look-ups of phase D run) and minpts 2 unless a test says otherwise."""
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
