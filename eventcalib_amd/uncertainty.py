"""Uncertainty of the solved intrinsics: the binding of include/ecal_uncertainty.h (the same libecal.so; design/24_uncertainty.md).

The prototypes of that header live here, in a table of their own, and are set on the handle of eventcalib_amd.load_library() by
apply_prototypes — capi.PROTOTYPES is the table of ecal.h and stays that.

    solver_uncertainty(solver, params, cluster_spans=1)   formal and cluster-robust covariance of fx fy cx cy k1..k5, a dict
    chunk_scores(solver, params)                          per-chunk sums of rho' r J [n_chunks, 33], of rho / 2, the chunk table
    uncertainty_map(cam_model, intr, cov, width, height)  per-pixel sigma of the bearing in pixels, on the host (no device)
    uncertainty_map_dev(ctx, ...)                         the same on the GPU, as torch tensors
"""
import ctypes

import numpy as np

from . import capi

INTRINSICS = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "k5")


class UncertaintyOptions(ctypes.Structure):   # ecal_uncertainty_options
    _fields_ = [("cluster_spans", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class UncertaintyResult(ctypes.Structure):   # ecal_uncertainty_result
    _fields_ = [("n_res", ctypes.c_uint64), ("n_unknowns", ctypes.c_uint32), ("n_cp", ctypes.c_uint32), ("n_chunks", ctypes.c_uint32),
                ("n_clusters", ctypes.c_uint32), ("positive_definite", ctypes.c_uint32), ("formal_valid", ctypes.c_uint32),
                ("robust_valid", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("cost", ctypes.c_double), ("s2", ctypes.c_double),
                ("cov", ctypes.c_double * 81), ("sigma", ctypes.c_double * 9), ("corr", ctypes.c_double * 81),
                ("cov_robust", ctypes.c_double * 81), ("sigma_robust", ctypes.c_double * 9), ("inflation", ctypes.c_double * 9)]


_P = ctypes.c_void_p
PROTOTYPES = {
    "ecal_solver_chunk_scores_dev": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "ecal_solver_chunk_scores": (ctypes.c_int, [_P, _P, _P, _P]),
    "ecal_solver_chunk_table": (ctypes.c_int, [_P, _P]),
    "ecal_uncertainty_default_options": (None, [ctypes.POINTER(UncertaintyOptions)]),
    "ecal_solver_uncertainty": (ctypes.c_int, [_P, _P, ctypes.POINTER(UncertaintyOptions), ctypes.POINTER(UncertaintyResult)]),
    "ecal_uncertainty_map_host": (ctypes.c_int, [ctypes.c_int, _P, _P, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P]),
    "ecal_uncertainty_map_dev": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P]),
}

_applied = None


def apply_prototypes(L):
    """the one place a prototype of ecal_uncertainty.h is set on a library handle (a missing symbol raises AttributeError)"""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def library():
    """libecal.so with this module's prototypes in place"""
    global _applied
    L = capi.load_library()
    if _applied is not L:
        _applied = apply_prototypes(L)
    return L


def _params(solver, params):
    p = np.ascontiguousarray(params, np.float64)
    assert p.shape == (solver.n_params,)
    return p


def chunk_table(solver):
    """ecal_solver_chunk_table: [n_chunks, 4] u32 = (cp0, count, seg, span)"""
    L = library()
    t = np.zeros((max(solver.n_chunks, 1), 4), np.uint32)
    solver.ctx._check(L.ecal_solver_chunk_table(solver._h, capi._ptr(t)))
    return t[:solver.n_chunks]


def chunk_scores(solver, params):
    """ecal_solver_chunk_scores: (score [n_chunks, 33], half_rho [n_chunks], table [n_chunks, 4])"""
    L = library()
    p = _params(solver, params)
    n = solver.n_chunks
    score = np.zeros((max(n, 1), 33))
    hr = np.zeros(max(n, 1))
    solver.ctx._check(L.ecal_solver_chunk_scores(solver._h, capi._ptr(p), capi._ptr(score), capi._ptr(hr)))
    return score[:n], hr[:n], chunk_table(solver)


def chunk_scores_dev(solver, d_params, d_score, d_half_rho=None, stream=0):
    """ecal_solver_chunk_scores_dev: raw device pointers, no host synchronisation"""
    solver.ctx._check(library().ecal_solver_chunk_scores_dev(solver._h, d_params, d_score, d_half_rho, stream))


def solver_uncertainty(solver, params, cluster_spans=1):
    """ecal_solver_uncertainty at `params`: a dict of the result's members (matrices as [9, 9] arrays, vectors [9]; the order of the
    nine is INTRINSICS), the flags as bools."""
    L = library()
    p = _params(solver, params)
    opt = UncertaintyOptions()
    L.ecal_uncertainty_default_options(ctypes.byref(opt))
    opt.cluster_spans = int(cluster_spans)
    res = UncertaintyResult()
    solver.ctx._check(L.ecal_solver_uncertainty(solver._h, capi._ptr(p), ctypes.byref(opt), ctypes.byref(res)))
    out = dict(n_res=int(res.n_res), n_unknowns=int(res.n_unknowns), n_cp=int(res.n_cp), n_chunks=int(res.n_chunks),
               n_clusters=int(res.n_clusters), cluster_spans=int(opt.cluster_spans), positive_definite=bool(res.positive_definite),
               formal_valid=bool(res.formal_valid), robust_valid=bool(res.robust_valid), cost=float(res.cost), s2=float(res.s2),
               names=INTRINSICS)
    for name in ("cov", "corr", "cov_robust"):
        out[name] = np.array(getattr(res, name)).reshape(9, 9)
    for name in ("sigma", "sigma_robust", "inflation"):
        out[name] = np.array(getattr(res, name))
    return out


def _map_args(cam_model, intr, cov, width, height):
    model = capi.CAMERA_FISHEYE if cam_model in (capi.CAMERA_FISHEYE, "fisheye", True) else capi.CAMERA_RADIAL
    k = np.ascontiguousarray(intr, np.float64).ravel()
    c = np.ascontiguousarray(cov, np.float64).ravel()
    assert k.shape == (9,) and c.shape == (81,)
    return model, k, c, int(width), int(height)


def uncertainty_map(cam_model, intr, cov, width, height, jacobian=False):
    """ecal_uncertainty_map_host: (sigma_px [height, width] f64, flag [height, width] u8); jacobian=True adds J [height, width, 2, 9]"""
    L = library()
    model, k, c, w, h = _map_args(cam_model, intr, cov, width, height)
    n = max(w, 0) * max(h, 0)
    sig = np.zeros(max(n, 1))
    flag = np.zeros(max(n, 1), np.uint8)
    jac = np.zeros(max(n, 1) * 18) if jacobian else None
    st = L.ecal_uncertainty_map_host(model, capi._ptr(k), capi._ptr(c), w, h, capi._ptr(sig), capi._ptr(flag), capi._ptr(jac) if jacobian else None)
    if st != 0:
        raise capi.EcalError(st, L.ecal_strerror(st).decode() + ": ecal_uncertainty_map_host (fx, fy above 0; width, height from 1 to 8192)")
    out = (sig[:n].reshape(h, w), flag[:n].reshape(h, w))
    return out + (jac[:18 * n].reshape(h, w, 2, 9),) if jacobian else out


def uncertainty_map_dev(ctx, cam_model, intr, cov, width, height, stream=0):
    """ecal_uncertainty_map_dev: (sigma_px f64 [height, width], flag u8 [height, width]) as CUDA tensors on the context's device"""
    import torch
    L = library()
    model, k, c, w, h = _map_args(cam_model, intr, cov, width, height)
    dev = torch.device("cuda", ctx.device)
    sig = torch.zeros((max(h, 1), max(w, 1)), dtype=torch.float64, device=dev)
    flag = torch.zeros((max(h, 1), max(w, 1)), dtype=torch.uint8, device=dev)
    ctx._check(L.ecal_uncertainty_map_dev(ctx._h, model, capi._ptr(k), capi._ptr(c), w, h, sig.data_ptr(), flag.data_ptr(), stream))
    return sig, flag


# the same as methods of capi.Solver
capi.Solver.uncertainty = solver_uncertainty
capi.Solver.chunk_scores = chunk_scores
capi.Solver.chunk_table = chunk_table
