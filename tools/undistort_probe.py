"""Measure the undistortion passes (design/20_undistort.md, design/09_measured.md) on the n-event synthetic 346 x 260 stream, with HIP
events, medians of --runs runs behind --warmup runs, in one process on one stream, the calls alternating inside every run:
  - ecal_undistort_events_dev, SUBPIXEL and PIXEL (the reference canvas), with the stream's own camera in the inverse form
    (ecal_inverse_radial_distortion of the synthetic lens), and ecal_undistort_points_dev
  - ecal_filter_events_dev with an empty mask (every event kept): the nearest existing pass — same verdict, scan and write shape —,
    unchanged from the parent commit: the yardstick
  - the passes of both (verdict, scan, write) from the library's own device events (ECAL_TRACE=load), in runs of their own
  - ecal_undistorted_frames_dev for --windows windows of --window-ms behind window bounds and the slicer, on packed and on double
    segments, and the three calls together
and the bytes each pass has to move, so that the times read as a share of HBM bandwidth.  One JSON line.
usage: python tools/undistort_probe.py [--events 50000000] [--windows 64] [--window-ms 4] [--warmup 3] [--runs 10]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eventcalib_amd  # noqa: E402
import synth_stream as SS  # noqa: E402
from eventcalib_amd import capi  # noqa: E402
from eventcalib_amd.pipeline import DetectPipeline  # noqa: E402

W, H = 346, 260
PASSES = ("verdict", "scan", "write")


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


class Trace:
    """the library's phase lines (stderr) of the calls made inside the block, under ECAL_TRACE=load"""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        os.environ["ECAL_TRACE"] = "load"
        capi.sync_env()
        self.file = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        del os.environ["ECAL_TRACE"]
        capi.sync_env()
        self.file.seek(0)
        phases = {}
        for m in re.finditer(r"ecal %s ingest: (.+?)\s+([0-9.]+) ms" % re.escape(self.what), self.file.read().decode()):
            phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
        self.phases = {k: statistics.median(v) for k, v in phases.items()}


def probe(ctx, n, a):
    st = torch.cuda.current_stream().cuda_stream
    ev = SS.make_stream(n, device="cuda")
    res = {"events": n, "warmup": a.warmup, "runs": a.runs}
    b5 = capi.inverse_radial_distortion([SS.K1, SS.K2, SS.K3, 0.0])
    cam = capi.undistort_camera([SS.FX, SS.FY, SS.CX, SS.CY] + [float(v) for v in b5], capi.CAMERA_RADIAL)
    sub, pix = capi.undistort_options(), capi.undistort_options(sensor=(W, H))
    out = torch.empty(n * 25, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    tot = torch.empty(4, dtype=torch.int64, device="cuda")
    mask = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    uv = torch.empty(2 * n, dtype=torch.float64, device="cuda")
    flag = torch.empty(n, dtype=torch.uint8, device="cuda")
    calls = {
        "undistort_subpixel": lambda: ctx.undistort_events_dev(cam, sub, ev.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st),
        "undistort_pixel": lambda: ctx.undistort_events_dev(cam, pix, ev.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st),
        "filter_events": lambda: ctx.filter_events_dev(ev.data_ptr(), n, mask.data_ptr(), W, H, out.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st),
        "undistort_points": lambda: ctx.undistort_points_dev(cam, ev.data_ptr(), n, uv.data_ptr(), flag.data_ptr(), st),
    }
    res["ms"], res["ms_min_max"] = timed_together(calls, a.warmup, a.runs)
    for name in ("undistort_subpixel", "undistort_pixel", "filter_events"):
        calls[name]()
        torch.cuda.synchronize()
        res[name + "_totals"] = [int(v) for v in tot.cpu().numpy()]
        kept = int(cnt.item()) & 0xFFFFFFFF
        # what the three passes have to move: the verdict pass 16 (17 with the mask byte) + 1 per event, the writing pass 1 per event and
        # 25 + 25 per kept event
        moved = n * ((17 if name == "filter_events" else 16) + 1 + 1) + kept * 50
        res[name + "_bytes"] = moved
        res[name + "_gb_per_s"] = moved / res["ms"][name] / 1e6
    res["undistort_over_filter"] = {k: res["ms"][k] / res["ms"]["filter_events"] for k in ("undistort_subpixel", "undistort_pixel")}
    for name, what in (("undistort_subpixel", "undistort"), ("undistort_pixel", "undistort"), ("filter_events", "hot pixel filter")):
        with Trace(what) as tr:
            for _ in range(a.warmup + a.runs):
                calls[name]()
            torch.cuda.synchronize()
        res[name + "_passes_ms"] = {k: tr.phases.get(k) for k in PASSES}
    del out, uv, flag
    torch.cuda.empty_cache()

    # ---- the frames: --windows windows spread over the stream
    S = a.windows
    t_first, t_last = 5.0, 5.0 + (n - 1) / 1e6
    t0 = t_first + (t_last - t_first - a.window_ms * 1e-3) * np.arange(S) / max(1, S - 1)
    t1 = t0 + a.window_ms * 1e-3
    cw, ch = int(pix.out_width), int(pix.out_height)
    rgb = torch.empty(S * ch * cw * 3, dtype=torch.uint8, device="cuda")
    ftot = torch.empty((S, 4), dtype=torch.int32, device="cuda")
    pipes = {}
    for packed in (True, False):
        p = DetectPipeline(ctx, packed=packed, want_event_point=False)
        p.set_windows(t0, t1)
        p.run(ev, slice_only=True)
        pipes[packed] = p
    torch.cuda.synchronize()

    def frames(packed):
        p = pipes[packed]
        ctx.undistorted_frames_dev(cam, pix, p._xy.data_ptr(), p._pk() if packed else None, p.seg_off.data_ptr(), p.seg_cnt.data_ptr(), S,
                                   rgb.data_ptr(), ftot.data_ptr(), st)

    def chain():
        pipes[True].run(ev, slice_only=True)
        frames(True)

    ms, spread = timed_together({"frames_packed": lambda: frames(True), "frames_doubles": lambda: frames(False), "bounds_slice_frames": chain},
                                a.warmup, a.runs)
    res["ms"].update(ms)
    res["ms_min_max"].update(spread)
    frames(True)
    torch.cuda.synchronize()
    f = ftot.cpu().numpy().astype(np.int64)
    res["frames"] = {"windows": S, "window_ms": a.window_ms, "canvas": [cw, ch], "points": int(f.sum()), "painted": int(f[:, :2].sum()),
                     "invalid": int(f[:, 2].sum()), "outside": int(f[:, 3].sum()), "rgb_bytes": S * ch * cw * 3,
                     "packed_segments": int((pipes[True].seg_fmt[: 2 * S] & 1).sum().item())}
    res["frames"]["rgb_gb_per_s"] = res["frames"]["rgb_bytes"] / res["ms"]["frames_packed"] / 1e6
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--window-ms", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    with eventcalib_amd.Context(0) as ctx:
        probe(ctx, a.events, a)


if __name__ == "__main__":
    main()
