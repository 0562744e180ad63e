"""Host only: the scaled synthetic scene leaves the default sensor's stream untouched, and the radius threshold the driver now
derives from the sensor's size is, at 346 x 260, the literal every default carries."""
import numpy as np

import synth_sensor as SN
import synth_stream as SS


def test_default_sensor_gives_the_same_bytes():
    plain = SS.make_stream(20000, rate=2.0e6, device="cpu", seed=31).numpy().copy()
    before = (SS.SENSOR_W, SS.SENSOR_H, SS.FX, SS.FY, SS.CX, SS.CY, SS.TRAJECTORY)
    with SN.sensor(346, 260) as s:
        assert s == 1.0
        same = SS.make_stream(20000, rate=2.0e6, device="cpu", seed=31).numpy().copy()
    assert np.array_equal(plain, same)
    with SN.sensor(640, 480, "orbit") as s:
        assert s == min(640 / 346, 480 / 260) and SS.TRAJECTORY == "orbit" and SS.FX == SS.FY == SN.BASE_FX * s
        _, xy, _ = SS.unpack_records(SS.make_stream(20000, rate=2.0e6, device="cpu", seed=31))
        xy = xy.numpy()
        assert xy.min() >= 0 and xy[:, 0].max() == 639 and xy[:, 1].max() == 479
    assert (SS.SENSOR_W, SS.SENSOR_H, SS.FX, SS.FY, SS.CX, SS.CY, SS.TRAJECTORY) == before
    assert np.array_equal(plain, SS.make_stream(20000, rate=2.0e6, device="cpu", seed=31).numpy())


def test_radius_threshold_of_the_default_sensor_is_the_literal():
    """ecal_circle_radius_threshold(346, 260, 9, 4, asymmetric, 5.5, 1.75), which calibrate_stream now hands to both detection
    passes, is bitwise the literal that DetectPipeline, detect_keyframes_device and capi's calls default to: the default path and
    the benchmark's results do not move by a bit.  (Host arithmetic of the library: no GPU.)"""
    import inspect
    from eventcalib_amd import adaptive, capi
    from eventcalib_amd.pipeline import DetectPipeline
    L = capi.load_library()
    thr = L.ecal_circle_radius_threshold(346.0, 260.0, 9, 4, 1, 5.5, 1.75)
    assert thr == 15.511363636363637
    for f in (DetectPipeline.set_detect_params, adaptive.detect_keyframes_device, adaptive.detect_keyframes, adaptive._detect_group,
              capi.detect_keyframes_dev, capi.detect_pass):
        assert inspect.signature(f).parameters["radius_threshold"].default == thr, f
    assert L.ecal_circle_radius_threshold(640.0, 480.0, 9, 4, 1, 5.5, 1.75) > 28.0      # a 640 x 480 sensor's is nearly twice that
