"""numpy restatements for the uncertainty tests (test infrastructure): the per-chunk score sums from ecal_residuals' own r and J with
the Huber loss restated, and the formal and cluster-robust covariance of the intrinsics from a dense normal matrix
(include/ecal_uncertainty.h).  Tangent order of every dense vector here: [intr 9 | per control point rot 3, trans 3]
(oracle_chain.dense_from_arrow)."""
import numpy as np

EPS = 2.0 ** -52


def huber_weight(r, a):
    """rho' of ceres::HuberLoss(a) at s = r^2, and rho / 2"""
    tail = ~(r * r <= a * a)
    w = np.where(tail, a / np.maximum(np.abs(r), 1e-300), 1.0)
    half_rho = np.where(tail, a * np.abs(r) - 0.5 * a * a, 0.5 * r * r)
    return w, half_rho, tail


def record_terms(solver, x):
    """(terms [n_res, 33] = rho' r J, half_rho [n_res], tail [n_res], cp0 [n_res]) from Solver.residuals at x"""
    r, J, cp0 = solver.residuals(x)
    w, half_rho, tail = huber_weight(r, solver.huber_a)
    return (w * r)[:, None] * J, half_rho, tail, cp0


def chunk_sums(terms, table):
    """the chunk table's record ranges (chunks lie one after another in record order) -> (sum [n_chunks, 33], sum of |terms|)"""
    start = np.concatenate([[0], np.cumsum(table[:, 1].astype(np.int64))])
    s = np.array([terms[start[c]:start[c + 1]].sum(axis=0) for c in range(len(table))]).reshape(len(table), terms.shape[1])
    a = np.array([np.abs(terms[start[c]:start[c + 1]]).sum(axis=0) for c in range(len(table))]).reshape(len(table), terms.shape[1])
    return s, a, start


def column_index(cp0):
    """dense tangent index of the 33 score columns of a chunk whose first control point is cp0"""
    idx = np.zeros(33, np.int64)
    idx[:9] = np.arange(9)
    for j in range(4):
        for k in range(3):
            idx[9 + 3 * j + k] = 9 + 6 * (cp0 + j) + k
            idx[21 + 3 * j + k] = 9 + 6 * (cp0 + j) + 3 + k
    return idx


def scatter(score, table, n_cp):
    """[n_chunks, 33] -> [n_chunks, 9 + 6 n_cp]"""
    out = np.zeros((len(table), 9 + 6 * n_cp))
    for c in range(len(table)):
        out[c, column_index(int(table[c, 0]))] = score[c]
    return out


def scaled_condition(H):
    """kappa_2 of the Jacobi-scaled matrix D H D, D = diag(1 / (1 + sqrt(diag)))"""
    d = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    return float(np.linalg.cond(H * d[:, None] * d[None, :])), d


def covariance(cost, H, n_res, score, table, n_cp, cluster_spans=1):
    """dict like uncertainty.solver_uncertainty's from the dense H (np.linalg.inv) and the chunk scores"""
    n = 9 + 6 * n_cp
    Hi = np.linalg.inv(H)
    Sii, P = Hi[:9, :9], Hi[:9, :]
    out = dict(n_unknowns=n, Sii=Sii, P=P)
    out["s2"] = 2.0 * cost / (n_res - n) if n_res > n else np.nan
    out["cov"] = out["s2"] * Sii
    out["sigma"] = np.sqrt(np.diag(out["cov"]))
    out["corr"] = out["cov"] / np.outer(out["sigma"], out["sigma"])
    g = scatter(score, table, n_cp)
    ids = [(int(t[2]), (int(t[3]) - 3) // cluster_spans) for t in table]
    uniq = sorted(set(ids))
    G = len(uniq)
    out["n_clusters"] = G
    S = np.array([P @ g[[i for i, k in enumerate(ids) if k == u]].sum(axis=0) for u in uniq]).reshape(G, 9)
    out["cov_robust"] = G / (G - 1) * S.T @ S if G >= 2 else np.full((9, 9), np.nan)
    out["sigma_robust"] = np.sqrt(np.diag(out["cov_robust"]))
    out["inflation"] = out["sigma_robust"] / out["sigma"]
    return out
