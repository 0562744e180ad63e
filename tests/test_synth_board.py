"""CPU: the synthetic boards of synth_board.py (the grid finder's ground truth at shapes other than 9 x 4) against things known
independently of it."""
import numpy as np
import pytest

import synth_board as SB


def test_9x4_reproduces_the_stream_generators_landmarks():
    import synth_stream as SS
    lm = SS.landmarks().numpy()
    assert (SS.ROWS, SS.COLS) == (9, 4)
    assert np.array_equal(SB.model_points(9, 4, SS.SQUARE), lm[:, :2]) and (lm[:, 2] == 0).all()
    # the convention, spelled out for a few indices of another shape: index i*cols + j -> (2j + i%2, i)
    p = SB.model_points(5, 3)
    assert p.shape == (15, 2)
    assert p[0].tolist() == [0, 0] and p[2].tolist() == [4, 0] and p[3].tolist() == [1, 1] and p[14].tolist() == [4, 4]


@pytest.mark.parametrize("rows", list(range(2, 17)))
def test_self_symmetries_follow_the_parity_of_rows(rows):
    """A half turn about the centroid, (x, y) -> (2 cols - 1 - x, rows - 1 - y), keeps x = 2j + i%2 on the lattice exactly when
    rows is even; the brute force over the point set must find that and nothing else."""
    for cols in (2, 3, 4, 7, 8):
        if rows * cols > 128:
            continue
        syms = SB.self_symmetries(rows, cols)
        M = rows * cols
        assert np.array_equal(syms[0], np.arange(M))
        if rows % 2:
            assert len(syms) == 1, (rows, cols)
        else:
            assert len(syms) == 2, (rows, cols)
            i, j = np.divmod(np.arange(M), cols)
            assert np.array_equal(syms[1], (rows - 1 - i) * cols + (cols - 1 - j))       # the half turn, index by index
            p = SB.model_points(rows, cols)
            assert np.allclose(p[syms[1]], np.array([2 * cols - 1, rows - 1]) - p)
    assert len(SB.self_symmetries(9, 4)) == 1


def _orientation(model, img):
    """sign of the determinant of the least-squares affine map model -> img, and of every small triangle's signed area"""
    A = np.concatenate([model, np.ones((len(model), 1))], axis=1)
    X, *_ = np.linalg.lstsq(A, img, rcond=None)
    return float(np.linalg.det(X[:2].T))


@pytest.mark.parametrize("shape", [(2, 2), (9, 4), (4, 11), (16, 8), (4, 27), (50, 2)])
def test_views_are_seen_from_the_front_at_the_wanted_step(shape):
    rows, cols = shape
    model = SB.model_points(rows, cols)
    for tilt, roll, seed in [(0, 0, 0), (0, 90, 1), (15, 200, 2), (30, 77, 3), (30, 301, 4)]:
        v = SB.views(rows, cols, None, 40.0, tilt, roll, seed)
        assert v.shape == (rows * cols, 2) and v.dtype == np.float64
        assert _orientation(model, v) > 0
        # ... locally too: the triangle (m, right neighbour, lower-right diagonal neighbour) keeps its sense everywhere
        for i in range(rows - 1):
            for j in range(cols - 1):
                a, b, c = v[i * cols + j], v[i * cols + j + 1], v[(i + 1) * cols + j + (i % 2)]
                assert (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) > 0
        assert abs(SB.nn_step(v) - 40.0) < 1e-9
        assert v.min() >= 4 * 40.0 - 1e-6                                               # the default image holds the board
    # frontal, no roll: the model itself, scaled (nearest neighbours are the diagonal ones, sqrt(2) model units apart)
    v = SB.views(rows, cols, None, 40.0, 0.0, 0.0, 0)
    assert np.allclose(v - v[0], (model - model[0]) * 40.0 / np.sqrt(2.0), atol=1e-6)
    # a given image: the projections' box is centred in it
    v = SB.views(rows, cols, (3000.0, 2000.0), 12.0, 20.0, 45.0, 5)
    assert np.allclose(0.5 * (v.min(axis=0) + v.max(axis=0)), [1500.0, 1000.0])


@pytest.mark.parametrize("k", [1, 2, 3, 8, 29, 92])
def test_ring_clutter_keeps_its_distances(k):
    rng = np.random.default_rng(k)
    pts = SB.views(9, 4, None, 40.0, 30.0, 10.0 * k, k) + rng.normal(0, 0.5, size=(36, 2))
    step = SB.nn_step(pts)
    c = SB.ring_clutter(pts, k, 3.0, rng)
    assert c.shape == (k, 2)
    assert np.linalg.norm(c[:, None] - pts[None], axis=2).min() >= 3.0 * step
    if k > 1:
        d = np.linalg.norm(c[:, None] - c[None], axis=2) + 1e12 * np.eye(k)
        assert d.min() >= 3.0 * step
        assert np.allclose(c.mean(axis=0), pts.mean(axis=0))                            # even in angle: the centroid stays
    allp = np.concatenate([pts, c])
    assert np.linalg.norm(allp - allp.mean(axis=0), axis=1).argmin() < 36               # the candidate nearest it: a circle
    assert SB.ring_clutter(pts, 0, 3.0, rng).shape == (0, 2)


def test_expected_orders_undo_the_shuffle_and_add_the_half_turn():
    rng = np.random.default_rng(0)
    perm = rng.permutation(40)
    (only,) = SB.expected_orders(perm, 9, 4)
    assert np.array_equal(perm[only], np.arange(36))
    a, b = SB.expected_orders(rng.permutation(50), 4, 11)
    assert sorted(a.tolist()) == sorted(b.tolist()) and np.array_equal(b, a[::-1])      # the half turn reverses the index
