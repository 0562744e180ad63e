"""GPU: the grid finder (ecal_grid_order_dev, eventcalib_amd/csrc/ecal_grid.hip) at pattern shapes other than 9 x 4 and with up to
128 candidates, against the synthetic boards of synth_board.py.

Every comparison is an exact integer comparison against synth_board.expected_orders: there is no numeric tolerance in this file.
Views are frontal to 30 degrees of tilt with a centre noise of sigma = 0.5 px unless a case says otherwise, and every case runs in
both launch forms — the default (a wave per start: few windows are at work) and ECAL_FORCE=grid_one_wave —, which must return
identical `order` and `found`.

The supported shapes (include/ecal.h): rows >= 2, cols >= 2, rows * cols <= 128 and cols - 1 + rows / 2 <= 28 — the longer span
of the board in lattice cells must fit the walk's window of 32 cells around a seed that is one cell off the middle at most.
Anything else is refused by the host with ECAL_ERR_INVALID before a kernel is launched."""
import os

import numpy as np
import pytest

import synth_board as SB

pytestmark = pytest.mark.gpu

FORMS = (None, "grid_one_wave")


def _supported(rows, cols):
    return rows >= 2 and cols >= 2 and rows * cols <= 128 and cols - 1 + rows // 2 <= 28


@pytest.fixture(scope="module")
def gpu():
    import torch
    import eventcalib_amd
    ctx = eventcalib_amd.Context(0)
    yield ctx, torch
    ctx.close()


def _each_form():
    """sets ECAL_FORCE for every launch form in turn (the sync_env() idiom: live contexts re-read their switches)"""
    from eventcalib_amd.capi import sync_env
    try:
        for form in FORMS:
            if form:
                os.environ["ECAL_FORCE"] = form
            else:
                os.environ.pop("ECAL_FORCE", None)
            sync_env()
            yield form
    finally:
        os.environ.pop("ECAL_FORCE", None)
        sync_env()


def _run_grid(ctx, torch, cand_lists, rows, cols, cap=128):
    """cand_lists: list of [n_i, 2] arrays -> (order [S, rows*cols], found [S])"""
    S, M = len(cand_lists), rows * cols
    xyr = np.zeros((S * cap, 3))
    info = np.zeros((S, 4), np.int32)
    seg_off = np.zeros(2 * S, np.int32)
    for s, p in enumerate(cand_lists):
        assert len(p) <= cap
        xyr[s * cap: s * cap + len(p), :2] = p
        xyr[s * cap: s * cap + len(p), 2] = 9.0
        info[s] = (len(p), 40, 40, 0)
        seg_off[2 * s], seg_off[2 * s + 1] = s * cap, s * cap + cap // 2
    d_xyr, d_info, d_off = torch.tensor(xyr).cuda(), torch.tensor(info).cuda(), torch.tensor(seg_off).cuda()
    order = torch.full((S, M), -7, dtype=torch.int32, device="cuda")
    found = torch.full((S,), -7, dtype=torch.int32, device="cuda")
    ctx.grid_order_dev(d_info.data_ptr(), d_off.data_ptr(), d_xyr.data_ptr(), S, rows, cols, order.data_ptr(), found.data_ptr(), 0)
    torch.cuda.synchronize()
    return order.cpu().numpy(), found.cpu().numpy()


def _run_both(ctx, torch, cand_lists, rows, cols, cap=128):
    """both launch forms; they must agree to the last entry"""
    outs = [_run_grid(ctx, torch, cand_lists, rows, cols, cap) for _ in _each_form()]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), \
        "%d x %d: the wave-per-start form and the one-wave form disagree" % (rows, cols)
    return outs[0]


def _case(rng, rows, cols, step=40.0, tilt=0.0, roll=0.0, sigma=0.5, clutter=0, min_steps=3.0, perm=None):
    """one window: (candidates [n, 2] = all[perm], perm, all); all[:M] are the board's circles in model order"""
    M = rows * cols
    pts = SB.views(rows, cols, None, step, tilt, roll, int(rng.integers(0, 1 << 30))) + rng.normal(0, sigma, size=(M, 2))
    allp = np.concatenate([pts, SB.ring_clutter(pts, clutter, min_steps, rng)])
    perm = rng.permutation(len(allp)) if perm is None else perm
    return allp[perm], perm, allp


def _seed_is_a_circle(cands, perm, M):
    """the candidate nearest the centroid of all candidates (the walk's first seed) is a circle of the board: a precondition of
    the case, checked on the CPU — if it fails the test is wrong, not the kernel"""
    return perm[int(np.linalg.norm(cands - cands.mean(axis=0), axis=1).argmin())] < M


def _is_expected(order_s, perm, rows, cols):
    return any(np.array_equal(order_s, e) for e in SB.expected_orders(perm, rows, cols))


def _assert_refused(ctx, torch, rows, cols):
    """ECAL_ERR_INVALID from the host check, with the shape and the limit in the text; nothing is launched: the outputs stay"""
    from eventcalib_amd.capi import EcalError
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    xyr = torch.zeros(3, dtype=torch.float64, device="cuda")
    order = torch.full((max(rows * cols, 1),), -7, dtype=torch.int32, device="cuda")
    found = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(EcalError) as e:
        ctx.grid_order_dev(z.data_ptr(), z.data_ptr(), xyr.data_ptr(), 1, rows, cols, order.data_ptr(), found.data_ptr(), 0)
    torch.cuda.synchronize()
    assert e.value.status == -1, (rows, cols)
    _names_shape_and_limit(str(e.value), rows, cols)
    assert int(found.cpu()[0]) == -7 and bool((order.cpu() == -7).all())


def _names_shape_and_limit(msg, rows, cols):
    assert "%d rows x %d cols" % (rows, cols) in msg, msg
    if rows < 2 or cols < 2:
        assert "at least 2 rows and 2 cols" in msg, msg
    elif rows * cols > 128:
        assert "rows * cols = %d, the limit is 128" % (rows * cols) in msg, msg
    else:
        assert "cols - 1 + rows / 2 = %d lattice cells, the limit is 28" % (cols - 1 + rows // 2) in msg, msg


def test_every_shape_is_found_in_four_rolls_or_refused_by_name(gpu):
    """Every (rows, cols) with rows, cols >= 2 and rows * cols <= 128: inside the supported bound the clean view at four in-plane
    rolls (0 / 90 / 180 / 270 degrees + a random offset; step 40 px, sigma 0.5 px; shuffled) is found with the pattern's order in
    all four windows, outside it the call is refused.  No shape is left out."""
    ctx, torch = gpu
    shapes = [(r, c) for r in range(2, 65) for c in range(2, 65) if r * c <= 128]
    inside = [sh for sh in shapes if _supported(*sh)]
    outside = [sh for sh in shapes if not _supported(*sh)]
    assert len(shapes) == len(inside) + len(outside) and len(shapes) > 300
    assert (4, 27) in inside and (3, 28) in inside and (2, 28) in inside and (55, 2) in inside and (5, 25) in inside
    assert (4, 28) in outside and (3, 29) in outside and (4, 32) in outside and (2, 64) in outside and (56, 2) in outside
    assert len(inside) == 326 and len(outside) == 64
    rng = np.random.default_rng(2024)
    windows = {}
    for rows, cols in inside:
        off = rng.uniform(0.0, 90.0)
        cs = [_case(rng, rows, cols, roll=q * 90.0 + off) for q in range(4)]
        for cands, perm, _ in cs:
            assert _seed_is_a_circle(cands, perm, rows * cols)
        windows[rows, cols] = cs
    outs = []
    for _ in _each_form():
        outs.append({sh: _run_grid(ctx, torch, [c[0] for c in cs], *sh) for sh, cs in windows.items()})
    lost, wrong, differ = [], [], []
    for sh, cs in windows.items():
        (o0, f0), (o1, f1) = outs[0][sh], outs[1][sh]
        if not (np.array_equal(o0, o1) and np.array_equal(f0, f1)):
            differ.append(sh)
        for w, (cands, perm, _) in enumerate(cs):
            if f0[w] != 1:
                lost.append(sh + (w,))
            elif not _is_expected(o0[w], perm, *sh):
                wrong.append(sh + (w,))
    print("\n[grid shapes] %d shapes found in four rolls, %d refused; lost %s, misordered %s, forms differ %s"
          % (len(inside), len(outside), lost[:20], wrong[:20], differ[:20]))
    assert not differ, "the two launch forms disagree at (rows, cols): %s" % differ[:20]
    assert not wrong, "misordered (rows, cols, window): %s" % wrong[:20]
    assert not lost, "not found (rows, cols, window): %s" % lost[:20]
    for rows, cols in outside:
        _assert_refused(ctx, torch, rows, cols)


def test_a_single_row_or_column_and_too_many_points_are_refused(gpu):
    """rows < 2 or cols < 2 is no grid the finder can orient; rows * cols > 128 does not fit.  A host check: no kernel runs."""
    ctx, torch = gpu
    for rows, cols in [(1, 4), (4, 1), (1, 36), (36, 1), (1, 128), (0, 4), (4, 0), (1, 1), (9, 15), (12, 11), (129, 1), (65, 2)]:
        _assert_refused(ctx, torch, rows, cols)


NAMED = [(2, 2), (3, 2), (2, 3), (3, 3), (5, 3), (11, 4), (4, 11), (7, 5), (10, 4), (16, 8), (8, 16), (32, 4), (15, 8),
         (4, 27), (3, 28),     # the two supported shapes nearest the bound (span 28) ...
         (4, 28), (3, 29)]     # ... and the two nearest it outside (span 29): refused


@pytest.mark.parametrize("shape", NAMED, ids=lambda sh: "%dx%d" % sh)
def test_named_shapes_with_tilt_and_clutter_off_the_board(gpu, shape):
    """Tilts of 0 / 15 / 30 degrees at a random roll, with min(8, 128 - M) false candidates on a ring three lattice steps outside
    the board: found, pattern order, every hole a true circle."""
    ctx, torch = gpu
    rows, cols = shape
    M = rows * cols
    if not _supported(rows, cols):
        _assert_refused(ctx, torch, rows, cols)
        return
    rng = np.random.default_rng(1000 * rows + cols)
    cs = [_case(rng, rows, cols, tilt=tilt, roll=rng.uniform(0, 360), clutter=min(8, 128 - M)) for tilt in (0.0, 15.0, 30.0) for _ in range(2)]
    for cands, perm, _ in cs:
        assert _seed_is_a_circle(cands, perm, M), "test bug: the candidate nearest the centroid is no circle of the board"
    order, found = _run_both(ctx, torch, [c[0] for c in cs], rows, cols)
    for w, (cands, perm, _) in enumerate(cs):
        assert found[w] == 1, "%d x %d, window %d (tilt %d): not found" % (rows, cols, w, 15 * (w // 2))
        assert _is_expected(order[w], perm, rows, cols), "%d x %d, window %d (tilt %d): order" % (rows, cols, w, 15 * (w // 2))


def _perm_with_circles_up_high(rng, n, M):
    """a shuffle of n candidates (the first M are the circles) that puts circles on the last index and, where there are such
    indices, on index 65 and 113: beyond the first four / seven candidate registers of a lane"""
    perm = rng.permutation(n)
    for target in [t for t in (n - 1, 65, 113) if t < n]:
        if perm[target] >= M:
            low = int(np.flatnonzero(perm < M)[0])        # a circle at a low index changes places with the false candidate
            perm[target], perm[low] = perm[low], perm[target]
    return perm


@pytest.mark.parametrize("n", [36, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128])
def test_9x4_among_up_to_128_candidates(gpu, n):
    """9 x 4 padded with ring clutter to n candidates: every count at which a lane's next candidate register comes into use
    (n = 16 k + 1), with circles of the board on the indices above 64 and above 112."""
    ctx, torch = gpu
    rng = np.random.default_rng(n)
    cs = []
    for tilt in (0.0, 15.0, 30.0):
        perm = _perm_with_circles_up_high(rng, n, 36)
        cs.append(_case(rng, 9, 4, tilt=tilt, roll=rng.uniform(0, 360), clutter=n - 36, perm=perm))
    for cands, perm, _ in cs:
        assert len(cands) == n and _seed_is_a_circle(cands, perm, 36)
        where = np.flatnonzero(perm < 36)
        assert n <= 36 or where.max() == n - 1
        assert n < 66 or (where > 64).any()
        assert n < 114 or (where > 112).any()
    order, found = _run_both(ctx, torch, [c[0] for c in cs], 9, 4)
    for w, (cands, perm, _) in enumerate(cs):
        assert found[w] == 1, "n = %d, window %d: not found" % (n, w)
        assert np.array_equal(order[w], np.argsort(perm)[:36]), "n = %d, window %d: order" % (n, w)


def test_129_candidates_are_more_than_the_kernel_handles(gpu):
    """the kernel's stated rule: more than 128 candidates -> found = 0, all -1 (next to a window of 128 that is found)"""
    ctx, torch = gpu
    rng = np.random.default_rng(129)
    a = _case(rng, 9, 4, tilt=15.0, roll=40.0, clutter=129 - 36)
    b = _case(rng, 9, 4, tilt=15.0, roll=40.0, clutter=128 - 36)
    order, found = _run_both(ctx, torch, [a[0], b[0]], 9, 4, cap=160)
    assert found[0] == 0 and (order[0] == -1).all()
    assert found[1] == 1 and np.array_equal(order[1], np.argsort(b[1])[:36])


@pytest.mark.parametrize("shape", [(16, 8), (15, 8)], ids=lambda sh: "%dx%d" % sh)
def test_128_candidates_at_the_largest_boards(gpu, shape):
    """16 x 8: the 128 circles and nothing else; 15 x 8: 120 circles + 8 false candidates.  Every candidate register, every
    index byte, every `occ` value up to 128 is in use."""
    ctx, torch = gpu
    rows, cols = shape
    M = rows * cols
    rng = np.random.default_rng(M)
    cs = [_case(rng, rows, cols, tilt=tilt, roll=rng.uniform(0, 360), clutter=128 - M) for tilt in (0.0, 15.0, 30.0)]
    for cands, perm, _ in cs:
        assert len(cands) == 128 and _seed_is_a_circle(cands, perm, M)
    order, found = _run_both(ctx, torch, [c[0] for c in cs], rows, cols)
    for w, (cands, perm, _) in enumerate(cs):
        assert found[w] == 1, "window %d: not found" % w
        assert _is_expected(order[w], perm, rows, cols), "window %d: order" % w
        assert order[w].max() >= 112


def _inner_circles(rows, cols):
    """circles with two rows above and below and a neighbour on either side in their own row (9 x 4: 9, 10, 13, 14, ... as in
    test_gpu_grid.py)"""
    return [i * cols + j for i in range(2, rows - 2) for j in range(1, cols - 1)]


@pytest.mark.parametrize("shape", [(16, 8), (9, 4)], ids=lambda sh: "%dx%d" % sh)
def test_small_step_where_the_fractional_tolerance_governs(gpu, shape):
    """step 12 px, sigma 0.3 px, frontal: the hole tolerance is min(20 px, 0.7 step) = 8.4 px, the fractional branch.  Clean views
    are found; an inner circle detected 0.5 step off its place along its row (6 px, far below 20 px) is accepted with that
    candidate in its place, one 0.9 step off (10.8 px, still below 20 px) leaves its hole empty: no grid.  (The analogue of the
    15 px / 25 px cases of test_grid_verdicts_on_incomplete_and_ambiguous_candidate_sets, in steps.)"""
    ctx, torch = gpu
    rows, cols = shape
    M = rows * cols
    rng = np.random.default_rng(12 * M)
    step = 12.0
    inner = _inner_circles(rows, cols)
    cases, expect = [], []
    for w in range(12):
        roll = rng.uniform(0, 360)
        seed = int(rng.integers(0, 1 << 30))
        truth = SB.views(rows, cols, None, step, 0.0, roll, seed)
        assert 0.7 * SB.nn_step(truth) < 20.0
        p = truth + rng.normal(0, 0.3, size=(M, 2))
        kind = w % 3
        if kind:
            k = inner[int(rng.integers(0, len(inner)))]
            row = (truth[k + 1] - truth[k]) / np.linalg.norm(truth[k + 1] - truth[k])
            p[k] = truth[k] + (0.5 if kind == 1 else 0.9) * step * row
        perm = rng.permutation(M)
        cases.append(p[perm])
        expect.append((kind, perm))
    order, found = _run_both(ctx, torch, cases, rows, cols)
    for w, (kind, perm) in enumerate(expect):
        if kind == 2:
            assert found[w] == 0 and (order[w] == -1).all(), "window %d: a circle 0.9 step off must leave its hole empty" % w
        else:
            assert found[w] == 1, "window %d (%s): not found" % (w, ("clean", "a circle 0.5 step off")[kind])
            assert _is_expected(order[w], perm, rows, cols), "window %d: order" % w


@pytest.mark.parametrize("shape", [(11, 4), (16, 8)], ids=lambda sh: "%dx%d" % sh)
def test_incomplete_boards_are_rejected(gpu, shape):
    """one circle missing, three far outliers added: n >= M candidates, but no complete grid -> found = 0, all -1"""
    ctx, torch = gpu
    rows, cols = shape
    M = rows * cols
    rng = np.random.default_rng(7 * M)
    cases = []
    for tilt in (0.0, 15.0, 30.0, 30.0):
        cands, perm, allp = _case(rng, rows, cols, tilt=tilt, roll=rng.uniform(0, 360))
        keep = np.delete(np.arange(M), int(rng.integers(0, M)))
        hi = allp.max(axis=0)
        far = hi + np.stack([rng.uniform(300, 340, 3), rng.uniform(0, 30, 3)], 1) + np.array([[0, 0], [60, 60], [120, 120]])
        q = np.concatenate([allp[keep], far])
        if len(q) > 128:
            q = q[:128]       # (16 x 8: 127 circles + one outlier)
        cases.append(q[rng.permutation(len(q))])
        assert len(cases[-1]) >= M
    order, found = _run_both(ctx, torch, cases, rows, cols)
    assert (found == 0).all() and (order == -1).all()


@pytest.mark.parametrize("shape", [(2, 2), (2, 3), (4, 11), (10, 4), (16, 8), (32, 4), (4, 27), (2, 28)], ids=lambda sh: "%dx%d" % sh)
def test_self_symmetric_boards_get_one_assignment_by_a_stated_rule(gpu, shape):
    """A board with an even number of rows maps onto itself under a half turn: two valid assignments.  Either passes above; here:
    both launch forms and a repeated call return the same one, and it is the one include/ecal.h states —

        the assignment in which the step from the seed (the candidate nearest the centroid of all candidates) to its nearest
        neighbour goes towards larger model x (one column step to the right on the board: from (x, y) to (x + 1, y +- 1)).

    Why: the walk's first basis vector is that step; match_pattern takes the first entry of its transform table that fits; entry 0
    (the identity) maps the walk's first axis to the model's (+1, +1) diagonal, entry 1 to (+1, -1), and for a self-symmetric board
    one of the two always fits, before the entries that map it to (-1, -1) and (-1, +1).  So the choice follows the candidates
    alone (through the noise on the seed's four diagonal neighbours), not the image's orientation: over the rolls below both
    assignments occur."""
    ctx, torch = gpu
    rows, cols = shape
    M = rows * cols
    assert len(SB.self_symmetries(rows, cols)) == 2
    rng = np.random.default_rng(M + 5)
    cs = [_case(rng, rows, cols, tilt=tilt, roll=rng.uniform(0, 360)) for tilt in (0.0, 0.0, 0.0, 0.0, 15.0, 15.0, 30.0, 30.0)]
    order, found = _run_both(ctx, torch, [c[0] for c in cs], rows, cols)
    again, found2 = _run_grid(ctx, torch, [c[0] for c in cs], rows, cols)
    assert np.array_equal(order, again) and np.array_equal(found, found2)
    model = SB.model_points(rows, cols)
    which = []
    for w, (cands, perm, _) in enumerate(cs):
        assert found[w] == 1, w
        exp = SB.expected_orders(perm, rows, cols)
        hit = [np.array_equal(order[w], e) for e in exp]
        assert sum(hit) == 1, w
        which.append(hit.index(True))
        seed = int(np.linalg.norm(cands - cands.mean(axis=0), axis=1).argmin())
        d = np.linalg.norm(cands - cands[seed], axis=1)
        d[seed] = np.inf
        nn = int(d.argmin())
        m_seed, m_nn = int(np.flatnonzero(order[w] == seed)[0]), int(np.flatnonzero(order[w] == nn)[0])
        assert model[m_nn, 0] - model[m_seed, 0] == 1.0 and abs(model[m_nn, 1] - model[m_seed, 1]) == 1.0, \
            "window %d: seed %s -> nearest neighbour %s" % (w, model[m_seed], model[m_nn])
    print("\n[grid shapes] %d x %d: assignment per window (0: identity, 1: half turn) %s" % (rows, cols, which))


def test_host_form_equals_device_form_at_other_shapes(gpu):
    """ecal_grid_order (one host candidate list) == ecal_grid_order_dev at 11 x 4 and 16 x 8; it refuses what the device form does"""
    from eventcalib_amd.capi import EcalError
    ctx, torch = gpu
    rng = np.random.default_rng(31)
    for rows, cols in [(11, 4), (16, 8)]:
        M = rows * cols
        cands, perm, _ = _case(rng, rows, cols, tilt=20.0, roll=123.0, clutter=min(8, 128 - M))
        xyr = np.concatenate([cands, np.full((len(cands), 1), 9.0)], axis=1)
        o_dev, f_dev = _run_both(ctx, torch, [cands], rows, cols)
        o_host, f_host = ctx.grid_order(xyr, rows, cols)
        assert f_host == 1 and f_dev[0] == 1 and np.array_equal(o_host, o_dev[0]) and _is_expected(o_host, perm, rows, cols)
        o_host, f_host = ctx.grid_order(xyr[: M - 1], rows, cols)          # fewer candidates than pattern points
        assert f_host == 0 and (o_host == -1).all()
    for rows, cols in [(4, 32), (2, 64), (1, 36), (4, 28)]:
        with pytest.raises(EcalError) as e:
            ctx.grid_order(np.zeros((128, 3)), rows, cols)
        assert e.value.status == -1
        _names_shape_and_limit(str(e.value), rows, cols)


def test_detection_entry_points_refuse_unsupported_shapes(gpu):
    """ecal_detect_pass, ecal_detect_keyframes and ecal_detect_stream_tiled validate rows x cols with the same helper, before any
    work: ECAL_ERR_INVALID, the shape and the limit in the text"""
    from eventcalib_amd import capi
    ctx, torch = gpu
    for rows, cols in [(4, 32), (1, 36), (3, 29)]:
        for call in (lambda: capi.detect_pass(ctx, None, 0, [0.0], [1.0], 1024, rows=rows, cols=cols),
                     lambda: capi.detect_keyframes_dev(ctx, None, 0, 0.01, 100, 2, 0.0, 1.0, 1024, 4, rows=rows, cols=cols),
                     lambda: capi.detect_stream_tiled(ctx, None, 0, 0.0, 0.01, 4, 16, rows=rows, cols=cols)):
            with pytest.raises(capi.EcalError) as e:
                call()
            assert e.value.status == -1
            _names_shape_and_limit(str(e.value), rows, cols)


def test_pipeline_order_grid_and_gather_features_at_11x4(gpu):
    """DetectPipeline.order_grid(11, 4) + gather_features(11, 4) on hand-written win_info / seg_off / cand_xyr buffers == a numpy
    gather: feat[s, k] = cand[order[s, k]] where a grid is found, NaN where none is or the window's status is not 0."""
    from eventcalib_amd.pipeline import DetectPipeline
    ctx, torch = gpu
    rows, cols, M, cap = 11, 4, 44, 64
    rng = np.random.default_rng(114)
    full = [_case(rng, rows, cols, tilt=t, roll=rng.uniform(0, 360), clutter=8) for t in (0.0, 25.0, 10.0, 30.0)]
    lists = [c[0] for c in full]
    lists[1] = np.delete(lists[1], int(np.flatnonzero(full[1][1] == 5)[0]), axis=0)     # window 1: circle 5 missing, 51 candidates
    status = [0, 0, 3, 0]                                                                 # window 2: failed an earlier stage
    S = len(lists)
    xyr = np.zeros((S * cap, 3))
    info = np.zeros((S, 4), np.int32)
    seg_off = np.zeros(2 * S, np.int32)
    for s, p in enumerate(lists):
        xyr[s * cap: s * cap + len(p), :2] = p
        xyr[s * cap: s * cap + len(p), 2] = 5.0 + 0.01 * np.arange(len(p)) + s          # every radius its own value
        info[s] = (len(p), 30, 30, status[s])
        seg_off[2 * s], seg_off[2 * s + 1] = s * cap, s * cap + 32
    pipe = DetectPipeline(ctx)
    pipe._ensure(S, S * cap)
    pipe.S = S
    pipe.win_info[:S].copy_(torch.tensor(info))
    pipe.seg_off[: 2 * S].copy_(torch.tensor(seg_off))
    pipe.cand_xyr[: S * cap].copy_(torch.tensor(xyr))
    res = []
    for _ in _each_form():
        order, found = pipe.order_grid(rows, cols)
        feat = pipe.gather_features(rows, cols)
        torch.cuda.synchronize()
        res.append((order.cpu().numpy().copy(), found.cpu().numpy().copy(), feat.cpu().numpy().copy()))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    order, found, feat = res[0]
    assert order.shape == (S, M) and feat.shape == (S, M, 3)
    assert found.tolist() == [1, 0, 0, 1]
    for s in range(S):
        if found[s]:
            assert _is_expected(order[s], full[s][1], rows, cols)
            assert np.array_equal(feat[s], xyr[s * cap + order[s]])
        else:
            assert (order[s] == -1).all() and np.isnan(feat[s]).all()
