"""Measure the hot-pixel filter's passes (design/17_hot_pixels.md, design/09_measured.md) on the n-event synthetic 346 x 260 stream,
with HIP events, medians of --runs runs behind --warmup runs:
  - the activity pass (ecal_pixel_activity_dev: the map's memset and pixel_activity_kernel) on the clean stream and on the same
    stream with every 40th event moved onto one of five pixels (the contention the feature is about)
  - the filter (ecal_filter_events_dev) with the five pixels masked, and with a random 30 % of the pixels masked; its verdict, scan
    and write passes from the library's own device events (ECAL_TRACE=load)
and, in the same run on the same stream, the passes of the parent commit they are held against:
  - ecal_solver_board_image_dev (the same record read and scattered u32 atomics, plus the FP64 pose work), with the ring profile and
    without it
  - ecal_solver_reassociate_dev (the same three-launch compaction, with the pose work in its verdict pass)
on a solver whose spline spans the stream's time range (tests/synth_solver.py's smooth trajectory, 20 control points a second), so
that every event is carried through a pose.  One JSON line.
usage: python tools/hot_pixel_probe.py [--events 50000000] [--warmup 3] [--runs 10]"""
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
os.environ["ECAL_TRACE"] = "load"
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eventcalib_amd  # noqa: E402
import synth_solver as SV  # noqa: E402
import synth_stream as SS  # noqa: E402
from eventcalib_amd import capi  # noqa: E402

W, H = 346, 260
HOT = [(3, 0), (120, 77), (200, 130), (345, 259), (17, 201)]


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
        for m in re.finditer(r"ecal (pixel activity|hot pixel filter) ingest: (.+?)\s+([0-9.]+) ms", self.file.read().decode()):
            phases.setdefault(m.group(2).strip(), []).append(float(m.group(3)))
        self.phases = {k: statistics.median(v) for k, v in phases.items()}


def probe(ctx, n, a):
    st = torch.cuda.current_stream().cuda_stream
    clean = SS.make_stream(n, device="cuda")
    hot = clean.clone()
    r = hot.view(n, 25)
    for k, (x, y) in enumerate(HOT):   # every 40th event onto one of five pixels: 2.5 % of the stream
        xy = torch.tensor([float(x), float(y)], dtype=torch.float64).view(torch.uint8).cuda()
        r[40 * k:: 200, 8:24] = xy
    res = {"events": n, "warmup": a.warmup, "runs": a.runs, "hot_events": int(sum(len(range(40 * k, n, 200)) for k in range(len(HOT))))}
    counts = torch.empty((2, H, W), dtype=torch.int32, device="cuda")
    tot = torch.empty(4, dtype=torch.int64, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    out = torch.empty(n * 25, dtype=torch.uint8, device="cuda")

    # ---- the activity pass
    for name, ev in (("clean", clean), ("hot", hot)):
        with Trace() as tr:
            res["activity_%s_ms" % name] = timed(lambda: ctx.pixel_activity_dev(ev.data_ptr(), n, W, H, counts.data_ptr(), tot.data_ptr(), st),
                                                 a.warmup, a.runs)
        res["activity_%s_kernel_ms" % name] = tr.phases.get("count")
    c = counts.cpu().numpy().view(np.uint32)
    mask5, info = capi.hot_pixel_mask(c)
    res["hot_pixels_found"] = info["n_hot_pixels"]
    assert sorted(zip(*np.nonzero(mask5))) == sorted((y, x) for x, y in HOT), "the rule must find the five pixels"

    # ---- the filter
    rng = np.random.default_rng(1)
    for name, ev, mask in (("hot_five_masked", hot, mask5), ("clean_30_percent_masked", clean, rng.random((H, W)) < 0.3)):
        d_mask = torch.from_numpy(mask.astype(np.uint8)).cuda()
        with Trace() as tr:
            res["filter_%s_ms" % name] = timed(lambda: ctx.filter_events_dev(ev.data_ptr(), n, d_mask.data_ptr(), W, H, out.data_ptr(), cnt.data_ptr(),
                                                                             tot.data_ptr(), st), a.warmup, a.runs)
        res["filter_%s_passes_ms" % name] = {k: tr.phases.get(k) for k in ("verdict", "scan", "write")}
        res["filter_%s_kept" % name] = int(cnt.item())
    del out, hot
    torch.cuda.empty_cache()

    # ---- the yardsticks: the parent commit's passes over the same records, a pose for every event
    t1 = 5.0 + n / 1e6
    prob, x = SV.make_problem(200, n_cp=max(12, int(20 * (t1 - 5.0))), t0=5.0, t1=t1, seed=1)
    solver = capi.Solver(ctx, prob)
    d_x = torch.from_numpy(x).cuda()
    for name, ring_bins in (("board_image", None), ("board_image_no_ring", 0)):
        o = solver.board_image_options(**({} if ring_bins is None else {"ring_bins": ring_bins}))
        img = torch.empty((2, int(o.height), int(o.width)), dtype=torch.int32, device="cuda")
        btot = torch.empty(7, dtype=torch.int64, device="cuda")
        rs = torch.empty((solver.n_landmarks, 2, 3), dtype=torch.float64, device="cuda")
        rh = torch.empty((solver.n_landmarks, max(int(o.ring_bins), 1)), dtype=torch.int64, device="cuda")
        res[name + "_ms"] = timed(lambda: solver.board_image_dev(d_x.data_ptr(), clean.data_ptr(), n, o, img.data_ptr(), btot.data_ptr(),
                                                                rs.data_ptr() if o.ring_bins else None, rh.data_ptr() if o.ring_bins else None, st),
                                  a.warmup, a.runs)
        res[name + "_totals"] = [int(v) for v in btot.cpu().numpy()]
    obs = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    tm = torch.empty(n, dtype=torch.float64, device="cuda")
    lm = torch.empty(n, dtype=torch.int32, device="cuda")
    sg = torch.empty(n, dtype=torch.int32, device="cuda")
    rtot = torch.empty(5, dtype=torch.int64, device="cuda")
    res["reassociate_ms"] = timed(lambda: solver.reassociate_dev(d_x.data_ptr(), clean.data_ptr(), n, 0.0, obs.data_ptr(), tm.data_ptr(), lm.data_ptr(),
                                                                sg.data_ptr(), cnt.data_ptr(), rtot.data_ptr(), st), a.warmup, a.runs)
    res["reassociate_totals"] = [int(v) for v in rtot.cpu().numpy()]
    solver.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    with eventcalib_amd.Context(0) as ctx:
        probe(ctx, a.events, a)


if __name__ == "__main__":
    main()
