"""The quality report's launch (memsets + report_kernel, every family on) against the cost-only evaluation (memsets +
normal_eq_kernel<with_jacobian = 0> + head reduction) of the same solver, on the benchmark's spline problem: device events, 5
warm-up and 20 timed runs each, the two alternating in three rounds."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import eventcalib_amd
from eventcalib_amd import capi
from eventcalib_amd.capi import Solver
import synth_solver_torch as ST
n_events = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
duration = n_events / 1e6
n_cp = max(4, int(duration / (50 * 5e-4)))
ctx = eventcalib_amd.Context(0)
prob, x = ST.make_problem(int(0.9 * n_events), n_cp, 5.0, 5.0 + duration, seed=777, device="cuda", round_pixels=True)
s = Solver(ctx, prob)
st = torch.cuda.current_stream()
d_x = torch.as_tensor(x, device="cuda")
d_acc = torch.empty(s.n_normal, dtype=torch.float64, device="cuda")
kf = np.arange(5.0 + 2e-3, 5.0 + duration, 4e-3)
d_kf = torch.as_tensor(kf, device="cuda")
o = s.report_options()
n_cells = -(-o.width // o.cell_px) * -(-o.height // o.cell_px)
d_total = torch.empty(7, dtype=torch.float64, device="cuda")
d_kfs = torch.empty(6 * len(kf), dtype=torch.float64, device="cuda")
d_lm = torch.empty(6 * s.n_landmarks, dtype=torch.float64, device="cuda")
d_cn = torch.empty(n_cells, dtype=torch.int64, device="cuda")
d_cs = torch.empty(n_cells, dtype=torch.float64, device="cuda")
d_h = torch.empty(o.hist_bins, dtype=torch.int64, device="cuda")
print("residuals %d chunks %d keyframes %d landmarks %d cells %d" % (s.n_res, s.n_chunks, len(kf), s.n_landmarks, n_cells), flush=True)


def cost_only():
    s.evaluate_dev(d_x.data_ptr(), 0, d_acc.data_ptr(), st.cuda_stream)


def report(fam=("kf", "lm", "cells", "hist")):
    s.report_dev(d_x.data_ptr(), d_kf.data_ptr(), len(kf), o, d_total.data_ptr(), d_kfs.data_ptr() if "kf" in fam else None,
                 d_lm.data_ptr() if "lm" in fam else None, d_cn.data_ptr() if "cells" in fam else None,
                 d_cs.data_ptr() if "cells" in fam else None, d_h.data_ptr() if "hist" in fam else None, st.cuda_stream)


def timed(fn, warm=5, runs=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(runs):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / runs


for rnd in range(3):
    a, b = timed(cost_only), timed(report)
    print("round %d: cost-only evaluation %.4f ms, report %.4f ms, ratio %.3f" % (rnd, a, b, b / a), flush=True)
# which family costs what: the report with one family at a time, and with none (totals only)
for fam in ((), ("kf",), ("lm",), ("cells",), ("hist",)):
    print("report with %-10s %.4f ms" % ("+".join(fam) or "totals only", timed(lambda: report(fam))), flush=True)
cost = d_acc[:1].cpu().numpy()[0]
report()
torch.cuda.synchronize()
tot = d_total.cpu().numpy().view(capi.REPORT_TOTALS)[0]
print("cost %.17g report cost %.17g n %d rms %.6g" % (cost, tot["cost"], tot["all"]["n"], np.sqrt(tot["all"]["sum_r2"] / tot["all"]["n"])))
