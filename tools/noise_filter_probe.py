"""Measure the noise filter's passes (design/19_noise_filter.md, design/09_measured.md) on the n-event synthetic 346 x 260 stream, with
HIP events, medians of --runs runs behind --warmup runs:
  - the verdict call (ecal_noise_verdict_dev) and the whole filter (ecal_denoise_events_dev) with the default options; the passes
    (keys, sort, index, support, count, scan, write) from the library's own device events (ECAL_TRACE=load), and the sort's share
  - the support pass at radius 2 and 3 and with include_self
and, in the same run on the same stream, two yardsticks:
  - ecal_stream_remove_hot_pixels (the parent commit's filter: count map, download, rule, upload, verdict, scan, write, a new stream),
    held against ecal_stream_remove_noise — wall time, both allocate the new stream's records
  - ecal_noise_verdict_host, the sequential walk on the host, on the first --host-events events, scaled to the stream
One JSON line.
usage: python tools/noise_filter_probe.py [--events 50000000] [--host-events 5000000] [--warmup 3] [--runs 10]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ECAL_TRACE"] = "load"
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eventcalib_amd  # noqa: E402
import synth_stream as SS  # noqa: E402
from eventcalib_amd import capi  # noqa: E402

W, H = 346, 260
PASSES = ("keys", "sort", "index", "support", "count", "scan", "write")


def timed(fn, warmup, runs):
    """median milliseconds between two HIP events around fn()"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def wall(fn, warmup, runs):
    """median wall milliseconds of fn() (calls that wait for the device themselves)"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


class Trace:
    """the library's phase lines (stderr) of the calls made inside the block"""

    def __enter__(self):
        self.file = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        phases = {}
        for m in re.finditer(r"ecal noise filter ingest: (.+?)\s+([0-9.]+) ms", self.file.read().decode()):
            phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
        self.phases = {k: statistics.median(v) for k, v in phases.items()}


def probe(ctx, n, a):
    st = torch.cuda.current_stream().cuda_stream
    ev = SS.make_stream(n, device="cuda")
    res = {"events": n, "warmup": a.warmup, "runs": a.runs}
    verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
    tot = torch.empty(4, dtype=torch.int64, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    out = torch.empty(n * 25, dtype=torch.uint8, device="cuda")
    o = capi.noise_options(width=W, height=H)

    # ---- the verdict call and the whole filter, defaults
    with Trace() as tr:
        res["verdict_ms"] = timed(lambda: ctx.noise_verdict_dev(ev.data_ptr(), n, o, verdict.data_ptr(), tot.data_ptr(), st), a.warmup, a.runs)
    res["verdict_passes_ms"] = {k: tr.phases.get(k) for k in PASSES[:4]}
    with Trace() as tr:
        res["denoise_ms"] = timed(lambda: ctx.denoise_events_dev(ev.data_ptr(), n, o, out.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st),
                                  a.warmup, a.runs)
    res["denoise_passes_ms"] = {k: tr.phases.get(k) for k in PASSES}
    known = [v for v in res["denoise_passes_ms"].values() if v is not None]
    if res["denoise_passes_ms"].get("sort") is not None and known:
        res["sort_share_of_passes"] = res["denoise_passes_ms"]["sort"] / sum(known)
    res["totals"] = [int(v) for v in tot.cpu().numpy()]
    res["kept"] = int(cnt.item())

    # ---- the support pass under other options
    for name, kw in (("radius2", dict(radius=2)), ("radius3", dict(radius=3)), ("radius3_support9", dict(radius=3, min_support=9)),
                     ("self", dict(include_self=1)), ("dt_1ms", dict(dt=1e-3))):
        ok = capi.noise_options(width=W, height=H, **kw)
        with Trace() as tr:
            res["verdict_%s_ms" % name] = timed(lambda: ctx.noise_verdict_dev(ev.data_ptr(), n, ok, verdict.data_ptr(), tot.data_ptr(), st),
                                                a.warmup, a.runs)
        res["support_%s_ms" % name] = tr.phases.get("support")
        res["removed_%s" % name] = int(tot[2].item())
    del out, verdict
    torch.cuda.empty_cache()

    # ---- yardstick 1: the library-owned stream calls, the parent commit's filter beside this one (wall time: both wait for the device)
    L = ctx._L
    vp = ctypes.c_void_p
    host = ev.cpu().numpy()
    h_in = vp()
    ctx._check(L.ecal_stream_create(ctx._h, host.ctypes.data, n, ctypes.byref(h_in)))
    hot_o = capi.hot_pixel_options(width=W, height=H)
    hot_info = capi.HotPixelInfo()
    ntot = np.zeros(1, capi.FILTER_TOTALS)

    def hot():
        h = vp()
        ctx._check(L.ecal_stream_remove_hot_pixels(ctx._h, h_in, ctypes.byref(hot_o), None, ctypes.byref(h), None, None, ctypes.byref(hot_info)))
        L.ecal_stream_destroy(h)

    def noise():
        h = vp()
        ctx._check(L.ecal_stream_remove_noise(ctx._h, h_in, ctypes.byref(o), ctypes.byref(h), ntot.ctypes.data))
        L.ecal_stream_destroy(h)

    res["stream_remove_hot_pixels_wall_ms"] = wall(hot, a.warmup, a.runs)
    res["stream_remove_noise_wall_ms"] = wall(noise, a.warmup, a.runs)
    res["stream_remove_noise_totals"] = [int(ntot[0][k]) for k in capi.FILTER_TOTALS.names]
    L.ecal_stream_destroy(h_in)

    # ---- yardstick 2: the sequential walk on the host, on the first events, scaled
    m = min(n, a.host_events)
    part = host[: m * 25]
    t0 = time.perf_counter()
    _, htot = capi.noise_verdict_host(part, width=W, height=H)
    res["host_walk_events"] = m
    res["host_walk_ms"] = (time.perf_counter() - t0) * 1e3
    res["host_walk_scaled_ms"] = res["host_walk_ms"] * n / m
    res["host_walk_removed"] = int(htot["n_removed"])
    res["device_verdict_speedup_over_host_walk"] = res["host_walk_scaled_ms"] / res["verdict_ms"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--host-events", type=int, default=5_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    with eventcalib_amd.Context(0) as ctx:
        probe(ctx, a.events, a)


if __name__ == "__main__":
    main()
