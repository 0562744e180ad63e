"""The synthetic scene of synth_stream on another sensor — test infrastructure.

`with sensor(W, H):` scales synth_stream's camera to a W x H sensor: the focal length by s = min(W / 346, H / 260), the
principal point to the sensor's centre ((W - 1) / 2, (H - 1) / 2: 172.5, 129.5 at 346 x 260), poses, board and distortion as
they are — the board covers the same share of the image, a circle's radius in pixels grows by s.  The module's values come back
on exit, the way the tests handle TRAJECTORY.  At (346, 260) nothing changes: make_stream gives the same bytes."""
import contextlib

import synth_stream as SS

BASE_W, BASE_H, BASE_FX = 346, 260, 359.67525


def scale(W, H):
    return min(W / BASE_W, H / BASE_H)


@contextlib.contextmanager
def sensor(W, H, trajectory=None):
    """Yields s.  trajectory: also set synth_stream.TRAJECTORY ("hover" / "orbit") for the block."""
    saved = (SS.SENSOR_W, SS.SENSOR_H, SS.FX, SS.FY, SS.CX, SS.CY, SS.TRAJECTORY)
    s = scale(W, H)
    try:
        SS.SENSOR_W, SS.SENSOR_H = int(W), int(H)
        SS.FX = SS.FY = BASE_FX * s
        SS.CX, SS.CY = (W - 1) / 2.0, (H - 1) / 2.0
        if trajectory is not None:
            SS.TRAJECTORY = trajectory
        yield s
    finally:
        SS.SENSOR_W, SS.SENSOR_H, SS.FX, SS.FY, SS.CX, SS.CY, SS.TRAJECTORY = saved


def project_centres(times):
    """The generating camera's circle centres [len(times), rows * cols, 2] at the given times (call inside sensor())."""
    import numpy as np
    import torch
    R, C = SS.pose(torch.as_tensor(np.asarray(times, np.float64)))
    lm = SS.landmarks()
    out = np.zeros((len(times), lm.shape[0], 2))
    for i in range(lm.shape[0]):
        out[:, i] = SS.project(lm[i][None, :].expand(len(times), 3), R, C).numpy()
    return out
