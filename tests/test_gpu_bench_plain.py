"""GPU: a plain `bench.py` run (no --full) — the headline line and nothing beside it, --steps timed passes, and --dump-outputs:
the same files from two runs on the same stream (3 and 4 timed passes), and kept clusters that add up to the oracle's on it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 2_000_000


def _plain(out_dir, steps=3):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--events", str(N_EVENTS), "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_line_and_outputs(tmp_path):
    a = _plain(tmp_path / "a", steps=3)
    b = _plain(tmp_path / "b", steps=4)
    for r, steps in ((a, 3), (b, 4)):
        assert r["metric"] == "Mevents/s DBSCAN+detect" and r["unit"] == "Mevents/s" and r["higher_is_better"] is True
        assert r["dtype"] == "f64" and r["steps"] == steps and r["failed_legs"] == []
        assert r["ms_per_step"] > 0 and abs(r["value"] - N_EVENTS / (r["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * r["value"]
        for side in ("roofline", "cpu_baseline", "pass_ms_fixed", "event_point_map", "median_ties", "h2d", "policy_p2", "solver",
                     "ingest", "init_calibration", "end_to_end", "weak_scaling"):
            assert side not in r, side
    da, db = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert da.keys() == db.keys() and {"win_info", "cand_xyr", "cand_pair", "rep", "xy", "labels", "kept_labels"} <= da.keys()
    for k in da:
        assert da[k].dtype == np.float64 and np.array_equal(da[k], db[k]), k
    assert sum(v.nbytes for v in da.values()) <= 64_000_000
    info = da["win_info"]
    assert info.shape == (a["config"]["windows_total"], 4) and da["cand_xyr"].shape[0] == a["config"]["circle_candidates"]
    assert (da["xy"] >= 0).all() and (da["xy"][:, 0] < 346).all() and (da["xy"][:, 1] < 260).all()
    assert (da["labels"] >= -1).all() and (da["kept_labels"] >= -1).all()
    # the dumped windows against the CPU oracle on the same stream (generated on the GPU, as bench.py does)
    import oracle_lib as O
    import synth_stream as SS
    ev = SS.make_stream(N_EVENTS, rate=1.0e6, t_start=5.0, seed=12345, device="cuda").cpu().numpy()
    t0, t1 = SS.tiled_windows(5.0, 5.0 + (N_EVENTS - 1) / 1.0e6, 1.5e-3)
    n_ev, kept = O.detect_windows(ev, t0, t1, 4.0, 2)
    assert n_ev == N_EVENTS and int(info[:, 1].sum() + info[:, 2].sum()) == kept
