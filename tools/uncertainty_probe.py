"""The uncertainty call on the benchmark's spline problem (45 M residuals at the default size): the chunk score kernel against the
evaluation with Jacobian (memsets + normal_eq_kernel<with_jacobian = 1> + head reduction) of the same solver — device events, 5
warm-up and 20 timed runs each, the two alternating in three rounds —, the whole ecal_solver_uncertainty call (wall clock, host part
included) and the sigma map at 346 x 260 and 1280 x 720."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import eventcalib_amd
from eventcalib_amd import capi, uncertainty
from eventcalib_amd.capi import Solver
import synth_solver_torch as ST
n_events = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
duration = n_events / 1e6
n_cp = max(4, int(duration / (50 * 5e-4)))
ctx = eventcalib_amd.Context(0)
prob, x = ST.make_problem(int(0.9 * n_events), n_cp, 5.0, 5.0 + duration, seed=777, device="cuda", round_pixels=True)
s = Solver(ctx, prob)
del prob
st = torch.cuda.current_stream()
d_x = torch.as_tensor(x, device="cuda")
d_acc = torch.empty(s.n_normal, dtype=torch.float64, device="cuda")
d_score = torch.empty((s.n_chunks, 33), dtype=torch.float64, device="cuda")
d_hr = torch.empty(s.n_chunks, dtype=torch.float64, device="cuda")
print("residuals %d control points %d chunks %d" % (s.n_res, s.n_cp, s.n_chunks), flush=True)


def evaluation():
    s.evaluate_dev(d_x.data_ptr(), 1, d_acc.data_ptr(), st.cuda_stream)


def scores():
    uncertainty.chunk_scores_dev(s, d_x.data_ptr(), d_score.data_ptr(), d_hr.data_ptr(), st.cuda_stream)


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
    a, b = timed(evaluation), timed(scores)
    print("round %d: evaluation with Jacobian %.4f ms, chunk scores %.4f ms, ratio %.3f" % (rnd, a, b, b / a), flush=True)
evaluation()
scores()
torch.cuda.synchronize()
print("cost %.17g sum half_rho %.17g; |sum of scores[:, fx]| %.6g against gradient[fx] %.6g" % (
    d_acc[0].item(), d_hr.sum().item(), d_score[:, 0].sum().item(), d_acc[1].item()), flush=True)
for spans in (1, 8):
    for k in range(3):
        t0 = time.perf_counter()
        u = uncertainty.solver_uncertainty(s, x, cluster_spans=spans)
        t1 = time.perf_counter()
        print("ecal_solver_uncertainty (cluster_spans %d), call %d: %.2f ms; clusters %d, positive definite %d, inflation %.3g .. %.3g" % (
            spans, k, 1e3 * (t1 - t0), u["n_clusters"], u["positive_definite"], np.nanmin(u["inflation"]), np.nanmax(u["inflation"])), flush=True)
print("sigma fx %.3g cx %.3g k1 %.3g | robust fx %.3g cx %.3g k1 %.3g" % (u["sigma"][0], u["sigma"][2], u["sigma"][4], u["sigma_robust"][0],
                                                                        u["sigma_robust"][2], u["sigma_robust"][4]), flush=True)
cov = u["cov_robust"] if u["robust_valid"] else u["cov"]
for w, h in ((346, 260), (1280, 720)):
    ms = timed(lambda: uncertainty.uncertainty_map_dev(ctx, capi.CAMERA_RADIAL, x[:9], cov, w, h, st.cuda_stream))
    t0 = time.perf_counter()
    sig, flag = uncertainty.uncertainty_map(capi.CAMERA_RADIAL, x[:9], cov, w, h)
    t1 = time.perf_counter()
    print("sigma map %d x %d: device %.4f ms (tensor allocation included), host %.2f ms; sigma_px %.3g .. %.3g, %d invalid" % (
        w, h, ms, 1e3 * (t1 - t0), sig[flag == 0].min(), sig.max(), int(flag.sum())), flush=True)
