"""GPU, small: the sharing modes of ecal_solver_solve (ecal_lm_options.distributed) with a few thousand residuals — time shards of one
spline at the 7 W <= n_cp edge (W = 2, n_cp = 14; W = 3, n_cp = 21) and distributed segments (W = 2, the problem of
test_two_segments), each against rank 0 solving the whole problem alone, with the tolerances bench.py's check_vs_single_solver is
held to (tests/test_gpu_bench_multirank.py, which runs the same modes at benchmark size); and the refusals, ECAL_ERR_INVALID on every
rank before any collective.  Ranks are spawned processes on the one GPU, their collectives run over gloo through
capi.make_allreduce_hook (bench.py's route under ECAL_BENCH_BACKEND=gloo)."""
import ctypes
import datetime
import os
import queue
import sys
import time

import numpy as np
import pytest

import synth_solver as SV

pytestmark = pytest.mark.gpu
ECAL_ERR_INVALID = -1
_child_died_by_signal = []     # once a child has ended by a signal nothing further is started on the GPU from here


def _last_solve(ctx, solver):
    how = (ctypes.c_uint32 * 8)()
    ctx._L.ecal_debug_solver_last_solve.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    ctx._check(ctx._L.ecal_debug_solver_last_solve(solver._h, how))
    return [int(v) for v in how]


INT_FIELDS = ("iterations", "successful_steps", "unsuccessful_steps", "jacobian_evaluations", "cost_evaluations", "termination")


def _record(ctx, solver, x, summ):
    return {"x": x, "summary": {f: int(getattr(summ, f)) for f in INT_FIELDS}, "final_cost": float(summ.final_cost),
            "last_solve": _last_solve(ctx, solver)[:7]}


def _sharded_options(solver, hook, mode, rank, world):
    opt = solver.default_options()
    opt.max_num_iterations = 12       # (as the streamed test: the stop tests do not sit on rounding)
    opt.allreduce = hook
    opt.distributed, opt.rank, opt.world_size = mode, rank, world
    return opt


def _solve_alone(capi, ctx, prob, x0):
    s = capi.Solver(ctx, prob)
    opt = s.default_options()
    opt.max_num_iterations = 12
    x, summ = s.solve(x0, opt)
    out = _record(ctx, s, x, summ)
    s.close()
    return out


def _time_shards(capi, ctx, hook, rank, world, calls):
    n_cp = 7 * world
    prob, x_gt = SV.make_problem(3000, n_cp=n_cp, seed=n_cp, pixel_noise=0.3)
    x0 = SV.perturb(x_gt, n_cp, np.random.default_rng(n_cp))
    cuts = np.concatenate([[-np.inf], capi.time_shard_cuts(prob["knots"], n_cp, world), [np.inf]])
    keep = (prob["time"] >= cuts[rank]) & (prob["time"] < cuts[rank + 1])
    s = capi.Solver(ctx, dict(prob, obs=prob["obs"][keep], time=prob["time"][keep], lm_id=prob["lm_id"][keep]))
    x, summ = s.solve(x0, _sharded_options(s, hook, 2, rank, world))
    out = dict(_record(ctx, s, x, summ), residuals=int(keep.sum()))
    s.close()
    if rank == 0:
        out["alone"] = _solve_alone(capi, ctx, prob, x0)
    return out


def _segments(capi, ctx, hook, rank, world, calls):
    n_cp = 6
    prob, x_gt = SV.make_problem(1200, n_cp=n_cp, seed=9, n_segments=world, pixel_noise=0.2)
    x0 = SV.perturb(x_gt, n_cp * world, np.random.default_rng(9))
    m = prob["seg_id"] == rank      # split as tests/test_multirank_gloo.py splits it: the rank's segment, the shared intrinsics
    mine = dict(prob, seg_cp_off=np.array([0, n_cp], np.uint32), knots=prob["knots"][10 * rank: 10 * rank + 10],
                obs=prob["obs"][m], time=prob["time"][m], lm_id=prob["lm_id"][m], seg_id=None)
    own = np.concatenate([np.arange(9), 9 + 4 * n_cp * rank + np.arange(4 * n_cp), 9 + 4 * n_cp * world + 3 * n_cp * rank + np.arange(3 * n_cp)])
    s = capi.Solver(ctx, mine)
    x, summ = s.solve(x0[own], _sharded_options(s, hook, 1, rank, world))
    out = dict(_record(ctx, s, x, summ), own=own)
    s.close()
    if rank == 0:
        out["alone"] = _solve_alone(capi, ctx, prob, x0)
    return out


def _refusals(capi, ctx, hook, rank, world, calls):
    """Every refusal comes back as ECAL_ERR_INVALID without a single call of the all-reduce; the ranks are still in step afterwards."""
    import torch.distributed as dist
    status = {}

    def refused(name, solver, x0, opt):
        try:
            solver.solve(x0, opt)
            status[name] = 0
        except capi.EcalError as e:
            status[name] = e.status

    n_cp = 7 * world - 1            # one control point short of 7 per rank
    prob, x_gt = SV.make_problem(600, n_cp=n_cp, seed=3, pixel_noise=0.3)
    s = capi.Solver(ctx, prob)
    refused("too few control points", s, x_gt, _sharded_options(s, hook, 2, rank, world))
    s.close()
    prob, x_gt = SV.make_problem(600, n_cp=7 * world, seed=3, pixel_noise=0.3)
    s = capi.Solver(ctx, prob)
    for mode in (1, 2):
        refused("rank == world, mode %d" % mode, s, x_gt, _sharded_options(s, hook, mode, world, world))
        refused("rank -1, mode %d" % mode, s, x_gt, _sharded_options(s, hook, mode, -1, world))
    # the library's own all-reduce with somebody else's context behind it
    other = capi.Context(0)
    opt = _sharded_options(s, hook, 2, rank, world)
    opt.allreduce, _ = ctx.comm_allreduce_fn()
    opt.allreduce_user = ctypes.cast(other._h, ctypes.c_void_p)
    refused("foreign allreduce_user", s, x_gt, opt)
    s.close()
    other.close()
    dist.barrier()
    return {"status": status, "allreduce_calls": calls[0]}


CASES = {"time_shards": _time_shards, "segments": _segments, "refusals": _refusals}


def _child(rank, world, port, case, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    # a collective that the other ranks never join ends with an error after this long (the hook then fails the solve)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from eventcalib_amd import capi
        ctx = capi.Context(0)
        inner = capi.make_allreduce_hook(ctx, world)
        calls = [0]

        def counted(user, d_buf, n, stream):
            calls[0] += 1
            return inner(user, d_buf, n, stream)

        hook = capi.ALLREDUCE_FN(counted)
        q.put((rank, None, CASES[case](capi, ctx, hook, rank, world, calls)))
        ctx.close()
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None))
    finally:
        dist.destroy_process_group()


def _run_ranks(case, world):
    """`world` (at most three) child processes; their results by rank.  A child that says nothing within the time limit is given up on;
    children that outlive the wait are terminated; after a child that ended by a signal nothing further is started."""
    import torch.multiprocessing as mp
    assert world <= 3
    if _child_died_by_signal:
        pytest.fail("not started: an earlier child process ended by signal %s" % _child_died_by_signal)
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = 29850 + os.getpid() % 100 + 100 * list(CASES).index(case) + world
    procs = [mpc.Process(target=_child, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, errors = {}, []
    deadline = time.monotonic() + 150
    while len(res) < world and time.monotonic() < deadline:
        try:
            rank, err, out = q.get(timeout=1.0)
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):    # a rank is gone without an answer: the others are not waited for
                break
            continue
        if err is not None:
            errors.append((rank, err))
        res[rank] = out
    if len(res) < world:
        errors.append(("parent", "no answer from ranks %s" % sorted(set(range(world)) - set(res))))
    for p in procs:
        p.join(timeout=30 if not errors else 5)
        if p.is_alive():
            p.terminate()
            p.join(timeout=10)
            errors.append(("parent", "rank process %d had to be terminated" % p.pid))
        elif p.exitcode is not None and p.exitcode < 0:
            _child_died_by_signal.append(-p.exitcode)
    assert not errors and not _child_died_by_signal, (errors, _child_died_by_signal)
    return [res[r] for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_time_shards_match_the_whole_problem_on_one_rank(world):
    res = _run_ranks("time_shards", world)
    xr, it, cost = res[0]["alone"]["x"], res[0]["alone"]["summary"]["iterations"], res[0]["alone"]["final_cost"]
    assert res[0]["alone"]["last_solve"][6] == 0
    assert sum(r["residuals"] for r in res) == 3000 and min(r["residuals"] for r in res) > 0
    for rank, r in enumerate(res):
        print("rank %d: iterations %d / %d, intrinsics %.3g, cost %.3g, control points %.3g" % (
            rank, r["summary"]["iterations"], it, np.abs(r["x"][:9] / xr[:9] - 1).max(), abs(r["final_cost"] / cost - 1), np.abs(r["x"][9:] - xr[9:]).max()))
        assert r["last_solve"][6] == 3 and r["last_solve"][5] == r["summary"]["iterations"]
        assert r["summary"]["iterations"] == it
        assert np.abs(r["x"][:9] / xr[:9] - 1).max() < 1e-8
        assert abs(r["final_cost"] / cost - 1) < 1e-9
        assert np.abs(r["x"][9:] - xr[9:]).max() < 1e-6
        assert np.array_equal(r["x"], res[0]["x"])          # every rank returns the same, complete solution


def test_distributed_segments_match_one_solver_over_both_segments():
    res = _run_ranks("segments", 2)
    xr, it, cost = res[0]["alone"]["x"], res[0]["alone"]["summary"]["iterations"], res[0]["alone"]["final_cost"]
    for rank, r in enumerate(res):
        ref = xr[r["own"]]
        print("rank %d: iterations %d / %d, intrinsics %.3g, cost %.3g, own control points %.3g" % (
            rank, r["summary"]["iterations"], it, np.abs(r["x"][:9] / ref[:9] - 1).max(), abs(r["final_cost"] / cost - 1), np.abs(r["x"][9:] - ref[9:]).max()))
        assert r["last_solve"][6] == 1 and r["last_solve"][5] == r["summary"]["iterations"]
        assert r["summary"]["iterations"] == it
        assert np.abs(r["x"][:9] / ref[:9] - 1).max() < 1e-8
        assert abs(r["final_cost"] / cost - 1) < 1e-9
        assert np.abs(r["x"][9:] - ref[9:]).max() < 1e-7
        assert np.array_equal(r["x"][:9], res[0]["x"][:9])  # all ranks return the same intrinsics


def test_refusals_come_before_any_collective():
    res = _run_ranks("refusals", 3)
    for r in res:
        assert len(r["status"]) == 6 and set(r["status"].values()) == {ECAL_ERR_INVALID}, r["status"]
        assert r["allreduce_calls"] == 0
