"""Measure image undistortion (design/22_image_undistort.md, design/09_measured.md) with HIP events, medians of --runs runs behind
--warmup runs, in one process on one stream, the calls alternating inside every run.  Per sensor (346 x 260 and 1280 x 720, 3
channels, the barrel camera of the tests scaled to the sensor, the reference canvas):
  - ecal_image_plan_create for both methods (wall time around the call: it waits for its own kernels and allocates the tables)
  - ecal_undistort_images_dev for --frames frames, REFERENCE (normalize 1: gather + finish) and BILINEAR (normalize 0: one launch;
    normalize 1: remap + finish)
  - ecal_copy_dev of the bytes an apply must read and write (the frames in, the pictures out): the HBM yardstick
and the table bytes per canvas pixel.  One JSON line.
usage: python tools/image_undistort_probe.py [--frames 256] [--warmup 3] [--runs 10]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import eventcalib_amd  # noqa: E402
from eventcalib_amd import capi  # noqa: E402

K_BARREL = [-0.21, 0.07, -0.012, 0.0011, -0.00004]
SENSORS = ((346, 260), (1280, 720))


def timed_together(fns, warmup, runs):
    """median milliseconds between two HIP events around each fn(), the fns alternating inside every run"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def probe_sensor(ctx, W, H, a):
    st = torch.cuda.current_stream().cuda_stream
    f = 251.3 * W / 346.0
    cam = capi.undistort_camera([f, f * 249.8 / 251.3, 171.2 * W / 346.0, 129.9 * H / 260.0] + K_BARREL, capi.CAMERA_RADIAL)
    N, C = a.frames, 3
    ref = capi.image_reference_options(W, H)
    opts = {"reference": ref,
            "bilinear": capi.image_options(sensor=(W, H), reference_canvas=True, method="bilinear", channels=C, normalize=0),
            "bilinear_normalized": capi.image_options(sensor=(W, H), reference_canvas=True, method="bilinear", channels=C, normalize=1)}
    ow, oh = int(ref.out_width), int(ref.out_height)
    res = {"sensor": [W, H], "canvas": [ow, oh], "frames": N, "channels": C}
    # the plans: wall milliseconds of a create + destroy, the median of --runs behind one warm-up
    build = {}
    for name in ("reference", "bilinear"):
        times = []
        for k in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan = ctx.image_plan(cam, W, H, opts[name])
            times.append((time.perf_counter() - t0) * 1e3)
            info = plan.info
            plan.close()
        build[name] = statistics.median(times[1:])
        res[name + "_plan"] = {k: info[k] for k in ("n_entries", "max_neighbours", "n_empty", "n_invalid", "n_not_converged", "bytes")}
        res[name + "_plan"]["bytes_per_canvas_pixel"] = info["bytes"] / float(ow * oh)
    res["plan_build_wall_ms"] = build
    src = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, device="cuda")
    dst = torch.empty((N, oh, ow, C), dtype=torch.uint8, device="cuda")
    in_bytes, out_bytes = src.numel(), dst.numel()
    scratch = torch.empty(in_bytes + out_bytes, dtype=torch.uint8, device="cuda")
    source = torch.empty(in_bytes + out_bytes, dtype=torch.uint8, device="cuda")
    plans = {k: ctx.image_plan(cam, W, H, o) for k, o in opts.items()}
    L = ctx._L

    def apply(name):
        ctx._check(L.ecal_undistort_images_dev(ctx._h, plans[name]._h, src.data_ptr(), N, dst.data_ptr(), None, st))

    calls = {name: (lambda name=name: apply(name)) for name in plans}
    # the yardstick: a device copy that reads as many bytes as an apply must read and writes as many as it must write
    calls["copy"] = lambda: ctx._check(L.ecal_copy_dev(ctx._h, scratch.data_ptr(), source.data_ptr(), max(in_bytes, out_bytes), st, 0))
    res["ms"], res["ms_min_max"] = timed_together(calls, a.warmup, a.runs)
    res["bytes"] = {"frames_in": in_bytes, "pictures_out": out_bytes, "copy_moves": 2 * max(in_bytes, out_bytes), "apply_must_move": in_bytes + out_bytes}
    res["copy_gb_per_s"] = res["bytes"]["copy_moves"] / res["ms"]["copy"] / 1e6
    res["apply_gb_per_s"] = {k: (in_bytes + out_bytes) / res["ms"][k] / 1e6 for k in plans}
    # an apply against the copy of the same useful bytes: the copy's time scaled to in + out bytes
    copy_same_bytes = res["ms"]["copy"] * (in_bytes + out_bytes) / res["bytes"]["copy_moves"]
    res["apply_over_copy"] = {k: res["ms"][k] / copy_same_bytes for k in plans}
    res["us_per_frame"] = {k: 1e3 * res["ms"][k] / N for k in plans}
    for p in plans.values():
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    with eventcalib_amd.Context(0) as ctx:
        out = {"warmup": a.warmup, "runs": a.runs, "sensors": [probe_sensor(ctx, W, H, a) for W, H in SENSORS]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
