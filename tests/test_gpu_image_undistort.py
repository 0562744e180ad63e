"""GPU: the image undistortion kernels (eventcalib_amd/csrc/ecal_image.hip) through capi.Context.image_plan, against the host walk
(ecal_undistort_image_host, ecal_image_table_host, ecal_image_maps_host, ecal_distort_points_host), which tests/
test_image_undistort_host.py holds against the numpy restatement.

Every camera and sensor of that file on the reference canvas, both methods, 1 and 3 channels, N = 1 and 5 (the odd N crosses the
four-frames-per-thread loop), normalize 0 and 1.  RADIAL is bit for bit: the table (first entries, indices, weight bits), the maps,
the pictures, every frame's min / max.  FISHEYE (tan, atan: a few ulp between libm and the device library): the same table entries,
weights within 1e-9 relative, maps within one f32 ulp, pictures at most one level apart in at most 0.5 % of the values; min / max
within 1e-5 relative (a weight off by 1e-9 relative moves an f32 average by an ulp or two of 1.2e-7).
B at 346 x 260 with N = 3 crosses a table of 1.1 million entries (4400 a workgroup of the counting pass) and a scan over 506 blocks."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_undistort_oracle as IO  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["B346", "B64", "B37", "P64", "F64", "I40"]
LEVEL_SHARE = 0.005
POSITION_TOL_PX = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


def lib_camera(name):
    from eventcalib_amd import capi
    cam, W, H = IO.camera(name)
    return capi.undistort_camera(cam["intr"], cam["model"]), cam, W, H


def options(W, H, **change):
    from eventcalib_amd import capi
    return capi.image_options(sensor=(W, H), reference_canvas=True, **change)


def frames(name, C, n):
    _, W, H = IO.camera(name)
    rng = np.random.default_rng(sum(name.encode()) * 8 + C)
    return rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def b32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_batch(c, W, H, o, batch):
    from eventcalib_amd import capi
    pics, mms = [], []
    for f in batch:
        pic, mm, _ = capi.undistort_image_host(c, W, H, f, o)
        pics.append(pic)
        mms.append(mm)
    return np.stack(pics), np.stack(mms)


def compare_pictures(name, got, mm, want, want_mm, what):
    if IO.CAMERAS[name][0] == 0:   # RADIAL
        assert (got == want).all(), what
        assert (b32(mm) == b32(want_mm)).all(), what
        return
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((diff > 0).mean())
    print("%s %s: %d of %d values differ (%.4f %%), at most %d level(s); min / max within %.2e relative"
          % (name, what, int((diff > 0).sum()), diff.size, 100.0 * share, int(diff.max()),
             float(np.abs(mm / np.where(want_mm != 0, want_mm, 1) - np.where(want_mm != 0, 1, mm)).max())))
    assert diff.max() <= 1 and share <= LEVEL_SHARE, what
    assert np.allclose(mm, want_mm, rtol=1e-5, atol=0.0), what


@pytest.mark.parametrize("name", NAMES)
def test_reference_plan_is_the_host_walk(ctx, name):
    from eventcalib_amd import capi
    c, cam, W, H = lib_camera(name)
    radial = cam["model"] == 0
    o = options(W, H)
    h_off, h_idx, h_w, h_info = capi.image_table_host(c, W, H, o)
    with ctx.image_plan(c, W, H, o) as plan:
        info = plan.info
        off, idx, w = plan.table()
        assert info["options"] == o.as_dict() and (info["width"], info["height"]) == (W, H)
        for k in ("n_invalid_sources", "n_empty", "n_entries", "max_neighbours"):
            assert int(info[k]) == int(h_info[k]), k
        assert info["bytes"] >= 4 * off.size + 12 * idx.size
        assert (off == h_off).all() and (idx == h_idx).all()
        if radial:
            assert (b64(w) == b64(h_w)).all()
        else:
            assert float(np.abs(w / h_w - 1.0).max()) <= 1e-9
        with pytest.raises(capi.EcalError) as e:
            plan.maps()
        assert e.value.status == -1 and "REFERENCE plan has no maps" in str(e.value)
    batch = {C: frames(name, C, 5) for C in (1, 3)}
    for C in (1, 3):
        for normalize in (0, 1):
            oc = options(W, H, channels=C, normalize=normalize)
            want, want_mm = host_batch(c, W, H, oc, batch[C])
            with ctx.image_plan(c, W, H, oc) as plan:
                for n in (1, 5):
                    got, mm = plan.apply(batch[C][:n], minmax=True)
                    assert got.shape == want[:n].shape
                    compare_pictures(name, got, mm, want[:n], want_mm[:n], "REFERENCE C=%d normalize=%d N=%d" % (C, normalize, n))


@pytest.mark.parametrize("name", NAMES)
def test_bilinear_plan_is_the_host_walk(ctx, name):
    from eventcalib_amd import capi
    c, cam, W, H = lib_camera(name)
    radial = cam["model"] == 0
    o = options(W, H, method="bilinear", channels=1, normalize=0)
    h_mx, h_my, h_valid, h_info = capi.image_maps_host(c, W, H, o)
    with ctx.image_plan(c, W, H, o) as plan:
        info = plan.info
        mx, my, valid = plan.maps()
        assert (valid == h_valid).all()
        for k in ("n_invalid", "n_not_converged", "n_empty", "truncated"):
            assert int(info[k]) == int(h_info[k]), k
        assert info["r_lim"] == h_info["r_lim"] and info["n_not_converged"] == 0
        ulps = max(int(np.abs(b32(mx).astype(np.int64) - b32(h_mx).astype(np.int64)).max()),
                   int(np.abs(b32(my).astype(np.int64) - b32(h_my).astype(np.int64)).max()))
        assert ulps <= (0 if radial else 1)
        dmx, dmy, dvalid = plan.maps_dev()
        assert (b32(dmx.cpu().numpy()) == b32(mx)).all() and (b32(dmy.cpu().numpy()) == b32(my)).all() and (dvalid.cpu().numpy() == valid).all()
        with pytest.raises(capi.EcalError) as e:
            plan.table()
        assert e.value.status == -1 and "BILINEAR plan has no table" in str(e.value)
    batch = {C: frames(name, C, 5) for C in (1, 3)}
    for C in (1, 3):
        for normalize in (0, 1):
            oc = options(W, H, method="bilinear", channels=C, normalize=normalize)
            want, want_mm = host_batch(c, W, H, oc, batch[C])
            with ctx.image_plan(c, W, H, oc) as plan:
                for n in (1, 5):
                    got, mm = plan.apply(batch[C][:n], minmax=True)
                    compare_pictures(name, got, mm, want[:n], want_mm[:n], "BILINEAR C=%d normalize=%d N=%d" % (C, normalize, n))
                    if not normalize:   # the launch that writes u8 straight out (no min / max asked)
                        direct = plan.apply(batch[C][:n])
                        assert (direct == got).all()


def test_barrel_346_x_260_three_frames_on_the_reference_canvas(ctx):
    """a table larger than one workgroup's share, the scan over many blocks, frames that do not fill the four-frame loop"""
    from eventcalib_amd import capi
    c, cam, W, H = lib_camera("B346")
    o = capi.image_reference_options(W, H)
    batch = frames("B346", 3, 3)
    with ctx.image_plan(c, W, H, o) as plan:
        info = plan.info
        assert info["n_entries"] == 1123163 and info["max_neighbours"] == 23 and info["n_empty"] == 52826   # (the numpy prototype's)
        assert (info["options"]["out_width"], info["options"]["out_height"]) == (415, 312)
        got, mm = plan.apply(batch, minmax=True)
    want, want_mm = host_batch(c, W, H, o, batch)
    assert (got == want).all() and (b32(mm) == b32(want_mm)).all()
    assert got.max() == 255 and (got == 0).mean() > 0.4


def test_apply_dev_equals_apply_and_a_plan_is_reusable(ctx):
    import torch
    c, cam, W, H = lib_camera("B64")
    for method in ("reference", "bilinear"):
        for normalize in (0, 1):
            o = options(W, H, method=method, channels=3, normalize=normalize)
            a, b = frames("B64", 3, 5), frames("P64", 3, 5)[::-1].copy()
            with ctx.image_plan(c, W, H, o) as plan:
                first, first_mm = plan.apply(a, minmax=True)
                other = plan.apply(b)
                again, again_mm = plan.apply(a, minmax=True)
                assert first.tobytes() == again.tobytes() and first_mm.tobytes() == again_mm.tobytes()
                assert other.tobytes() != first.tobytes()
                t = torch.from_numpy(a).cuda()
                dev, dev_mm = plan.apply_dev(t, minmax=True)
                assert dev.is_cuda and tuple(dev.shape) == first.shape
                assert dev.cpu().numpy().tobytes() == first.tobytes() and dev_mm.cpu().numpy().tobytes() == first_mm.tobytes()
                assert plan.apply_dev(t).cpu().numpy().tobytes() == first.tobytes()
                # an output that starts 1 and 3 bytes past a word boundary: the same bytes, nothing written in front or behind
                C, oh, ow = 3, int(o.out_height), int(o.out_width)
                nbytes = 5 * oh * ow * C
                for shift in (1, 3):
                    buf = torch.full((nbytes + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                    ctx._check(ctx._L.ecal_undistort_images_dev(ctx._h, plan._h, t.data_ptr(), 5, buf.data_ptr() + shift, None,
                                                                torch.cuda.current_stream().cuda_stream))
                    torch.cuda.synchronize()
                    h = buf.cpu().numpy()
                    assert h[shift:shift + nbytes].tobytes() == first.tobytes()
                    assert (h[:shift] == 0xAB).all() and (h[shift + nbytes:] == 0xAB).all()
                # one frame, (H, W, C) and (H, W) in, the same rank out
                assert plan.apply(a[0]).shape == (oh, ow, 3) and (plan.apply(a[0]) == first[0]).all()
                assert plan.apply(np.zeros((0, H, W, 3), np.uint8)).shape == (0, oh, ow, 3)
    o1 = options(W, H, method="bilinear", channels=1, normalize=0)
    with ctx.image_plan(c, W, H, o1) as plan:
        grey = frames("B64", 1, 1)[0, :, :, 0]
        out = plan.apply(grey)
        assert out.shape == (int(o1.out_height), int(o1.out_width)) and (out == plan.apply(grey[None, :, :, None])[0, :, :, 0]).all()


@pytest.mark.parametrize("name", NAMES)
def test_distort_points_on_the_device_are_the_host_s(ctx, name):
    from eventcalib_amd import capi
    c, cam, W, H = lib_camera(name)
    d = IO.reference_options(W, H)
    X, Y = np.meshgrid(np.arange(d["out_width"], dtype=np.float64), np.arange(d["out_height"], dtype=np.float64))
    grid = np.stack([X.ravel() - d["off_x"], Y.ravel() - d["off_y"]], axis=1)
    odd = np.array([[np.nan, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [-np.inf, np.inf], [1e300, 1e300], [1e6, -1e6],
                    [1e-300, 1e-300], [-0.0, 0.0], [17.25, 9.75], [-3.5, 40.125]])
    uv = np.concatenate([grid, grid[::5] + 0.37, odd])
    want, want_flag = capi.distort_points_host(c, W, H, uv)
    got, flag = ctx.distort_points(c, W, H, uv)
    got, flag = got.cpu().numpy(), flag.cpu().numpy()
    assert (flag == want_flag).all()
    if cam["model"] == 0:
        assert (b64(got) == b64(want)).all()
    else:
        assert float(np.abs(got - want).max()) <= POSITION_TOL_PX
    assert (flag[-11:-5] == capi.DISTORT_INVALID).all() and (got[-11:-5] == 0.0).all()
    assert ctx.distort_points(c, W, H, np.zeros((0, 2)))[0].shape == (0, 2)


def test_refusals_come_before_any_launch(ctx):
    import torch
    import eventcalib_amd
    from eventcalib_amd import capi
    c, cam, W, H = lib_camera("B346")
    o = options(W, H, method="bilinear", channels=1, normalize=0)
    L = ctx._L
    with ctx.image_plan(c, W, H, o) as plan:
        npix = int(o.out_width) * int(o.out_height)
        src = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(npix, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        n_range = (2 ** 32 - 1) // npix + 1     # 33 172 frames: above 2^32 - 1 frames x canvas pixels, below the frame limit
        assert n_range < 262140
        for n, text in ((n_range, "more than 2^32-1 frames x canvas pixels"), (262141, "more than")):
            st = L.ecal_undistort_images_dev(ctx._h, plan._h, src.data_ptr(), n, dst.data_ptr(), None, stream)
            assert st == -6 and text in L.ecal_last_error(ctx._h).decode()
        st = L.ecal_undistort_images(ctx._h, plan._h, ctypes.c_void_p(src.data_ptr()), n_range, ctypes.c_void_p(dst.data_ptr()), None)
        assert st == -6
        torch.cuda.synchronize()
        assert int(dst.sum().item()) == 0   # (nothing ran)
        for args in ((None, 1, dst.data_ptr()), (src.data_ptr(), 1, None)):
            st = L.ecal_undistort_images_dev(ctx._h, plan._h, args[0], args[1], args[2], None, stream)
            assert st == -1 and "null pointer" in L.ecal_last_error(ctx._h).decode()
        assert L.ecal_undistort_images_dev(ctx._h, None, src.data_ptr(), 1, dst.data_ptr(), None, stream) == -1
        with eventcalib_amd.Context(0) as other:
            st = L.ecal_undistort_images_dev(other._h, plan._h, src.data_ptr(), 1, dst.data_ptr(), None, stream)
            assert st == -1 and "another context" in L.ecal_last_error(other._h).decode()
        with pytest.raises(ValueError):
            plan.apply(np.zeros((H, W, 3), np.uint8))   # (a one-channel plan)
    for change, text in ((dict(method=2), "method must be"), (dict(channels=2), "channels must be 1 or 3"), (dict(out_width=8193), "out_width from 1 to 8192"),
                         (dict(out_height=0), "out_height from 1 to 8192"), (dict(normalize=2), "normalize must be 0 or 1"),
                         (dict(reserved=1), "options reserved must be 0"), (dict(off_x=np.nan), "off_x must be finite")):
        with pytest.raises(capi.EcalError) as e:
            ctx.image_plan(c, W, H, options(W, H, **change))
        assert e.value.status == -1 and "ecal_image_plan_create: " + text in str(e.value), change
    for w, h, text in ((0, H, "width from 1 to 8192"), (W, 8193, "height from 1 to 8192")):
        with pytest.raises(capi.EcalError) as e:
            ctx.image_plan(c, w, h, o)
        assert e.value.status == -1 and text in str(e.value)
        with pytest.raises(capi.EcalError) as e:
            ctx.distort_points(c, w, h, [[1.0, 2.0]])
        assert e.value.status == -1 and "ecal_distort_points: " + text in str(e.value)
    bad = capi.undistort_camera(cam["intr"], capi.CAMERA_RADIAL)
    bad.intr[5] = np.inf
    with pytest.raises(capi.EcalError) as e:
        ctx.image_plan(bad, W, H, o)
    assert e.value.status == -1 and "k2 must be finite" in str(e.value)


def test_calibrate_layer(ctx):
    from eventcalib_amd import calibrate, capi
    cam, W, H = IO.camera("B64")
    c = capi.undistort_camera(cam["intr"], cam["model"])
    batch = frames("B64", 3, 2)
    ref = calibrate.undistort_images(ctx, batch, cam["intr"], method="reference", canvas="reference")
    want, _ = host_batch(c, W, H, capi.image_reference_options(W, H), batch)
    assert ref.shape == want.shape and (ref == want).all()
    one = calibrate.undistort_images(ctx, batch[0], cam["intr"], method="bilinear")
    want1, _, _ = capi.undistort_image_host(c, W, H, batch[0], capi.image_options(sensor=(W, H), channels=3))
    assert one.shape == (H, W, 3) and (one == want1).all()
    grey = calibrate.undistort_images(ctx, batch[0, :, :, 1], cam["intr"], method="bilinear", out_width=70, out_height=50, off_x=3.0, off_y=1.0)
    wantg, _, _ = capi.undistort_image_host(c, W, H, np.ascontiguousarray(batch[0, :, :, 1]),
                                            capi.image_options(sensor=(W, H), out_width=70, out_height=50, off_x=3.0, off_y=1.0))
    assert grey.shape == (50, 70) and (grey == wantg).all()
    with pytest.raises(TypeError):
        calibrate.undistort_images(ctx, batch, cam["intr"], no_such_option=1)
    m = calibrate.undistort_maps(ctx, cam["intr"], capi.CAMERA_RADIAL, W, H, canvas="reference")
    mx, my, valid, info = capi.image_maps_host(c, W, H, capi.image_options(sensor=(W, H), reference_canvas=True, method="bilinear", channels=1, normalize=0))
    assert (b32(m["map_x"]) == b32(mx)).all() and (b32(m["map_y"]) == b32(my)).all() and (m["valid"] == valid).all()
    assert m["info"]["r_lim"] == info["r_lim"] and m["map_x"].shape == (58, 77)
