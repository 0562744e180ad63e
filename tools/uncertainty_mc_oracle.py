"""The CPU oracle of tests/test_gpu_uncertainty.py's Monte Carlo check, no GPU: one noise-free synth_solver problem (n_cp = 8), K = 256
seeded draws of iid pixel noise, each solved from the truth by tests/ref_lm.py (the dense restatement of the LM loop over the C++
oracle's evaluation), the formal covariance s2 (H^-1)_intr in numpy, and the mean over the draws of (x - truth)^T cov^-1 (x - truth)
against the band 9 +- 4 sqrt(18 / K) of a chi^2_9 mean.
  usage: python tools/uncertainty_mc_oracle.py N_RES SIGMA_PX [FIRST_SEED]      (the test's figures: 1024 0.005 1000 -> 9.279)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth_solver as SV, ref_lm, oracle_lib as O

N_RES, N_CP, K, SIGMA = int(sys.argv[1]), 8, 256, float(sys.argv[2])
SEED0 = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
prob, x_gt = SV.make_problem(N_RES, n_cp=N_CP, seed=9, pixel_noise=0.0)
n = 9 + 6 * N_CP
t0 = time.time()
stats = []
for k in range(K):
    rng = np.random.default_rng(SEED0 + k)
    p = dict(prob, obs=prob["obs"] + SIGMA * rng.normal(size=prob["obs"].shape))
    x, hist, it = ref_lm.solve(p, x_gt)
    cost, g, H = O.solver_evaluate(p, x)
    cov = 2 * cost / (N_RES - n) * np.linalg.inv(H)[:9, :9]
    d = x[:9] - x_gt[:9]
    stats.append(d @ np.linalg.solve(cov, d))
    if k % 64 == 0:
        print("draw %d: %d iterations, statistic %.4f, %.1f s" % (k, it, stats[-1], time.time() - t0), flush=True)
stats = np.array(stats)
half = 4 * np.sqrt(18 / K)
print("mean %.4f band %.4f .. %.4f std %.3f (a chi^2_9 has 4.243)" % (stats.mean(), 9 - half, 9 + half, stats.std()))
