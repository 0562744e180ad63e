"""Slice stage alone on a stream whose tiled windows hold more events than the bench stream's: HIP-event time of the staged
slice call (window bounds outside the timed span), for comparing two builds of libecal.so.  The default, 5 M events at 1.25 Mev/s in
tiled 1.5 ms windows, gives ~1875 events a window: the eight-slot form of the first hash pass (slice_hash.hpp).
python tools/slice_stage_time.py [events] [rate] [window_s] [repeats]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import eventcalib_amd
from eventcalib_amd.pipeline import DetectPipeline
import synth_stream as SS
n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
rate = float(sys.argv[2]) if len(sys.argv) > 2 else 1.25e6
wlen = float(sys.argv[3]) if len(sys.argv) > 3 else 1.5e-3
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 50
ctx = eventcalib_amd.Context(0); pipe = DetectPipeline(ctx)
ev = SS.make_stream(n, rate=rate, device="cuda")
t0, t1 = SS.tiled_windows(5.0, 5.0 + (n - 1) / rate, wlen)
pipe.set_windows(t0, t1)
S = len(t0)
for _ in range(3):
    pipe.run(ev, slice_only=True)
torch.cuda.synchronize()
sizes = (pipe.win_hi[:S] - pipe.win_lo[:S]).cpu()
st = torch.cuda.current_stream().cuda_stream
c = ctx
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):   # (the slice call alone: the bounds of the windows stay what the warm-up left)
    c.slice_events_packed_dev(ev.data_ptr(), n, pipe.win_lo.data_ptr(), pipe.win_hi.data_ptr(), pipe.win_base.data_ptr(), S, 0, n,
                              pipe._xy.data_ptr(), pipe.seg_off.data_ptr(), pipe.seg_cnt.data_ptr(), pipe.event_point.data_ptr(),
                              pipe.flags.data_ptr(), pipe._pk(), st)
e1.record(); torch.cuda.synchronize()
assert not pipe.overflowed()
print("rate %.2f Mev/s, window %.2f ms: %d events, %d windows of %d .. %d events (median %d, %d above 1535, %d above 2047), slice stage %.4f ms"
      % (rate / 1e6, wlen * 1e3, n, S, int(sizes.min()), int(sizes.max()), int(sizes.median()), int((sizes > 1535).sum()),
         int((sizes > 2047).sum()), e0.elapsed_time(e1) / reps))
