"""CPU: bench.py's --dump-outputs writer on a stand-in pipeline of host tensors — which slots of the pipeline's arrays it reads
(candidates and representatives of the windows that reached pairing, a seeded sample of the points), the float64 files, the
size budget, and that the same input gives the same files."""
import os

import numpy as np
import torch

import bench


class _Pipe:
    pass


def _pipe(S=600, seed=0):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 60, 2 * S)
    off = np.cumsum(np.concatenate([[0], (cnt + rng.integers(0, 5, 2 * S))[:-1]]))      # segments with gaps between them
    slots = int(off[-1] + cnt[-1] + 10)
    wi = np.zeros((S, 4), np.int64)
    wi[:, 3] = rng.choice([0, 1, 4, 0x100], S)                                         # ok, no pairing, capacity, ok + tie flag
    ok = (wi[:, 3] & 0xFF) == 0
    wi[ok, 1] = np.minimum(cnt[0::2][ok], 7)
    wi[ok, 2] = np.minimum(cnt[1::2][ok], 7)
    wi[ok, 0] = np.minimum(wi[ok, 1], wi[ok, 2])
    p = _Pipe()
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    p.seg_off, p.seg_cnt, p.win_info = i32(off), i32(cnt), i32(wi)
    p.n_clusters = i32(rng.integers(0, 9, 2 * S))
    p.win_lo = torch.arange(S, dtype=torch.int32)
    p.win_hi = p.win_lo + 5
    # every per-slot array holds a function of the slot number, so a read of the wrong slot shows
    p.labels = torch.arange(slots, dtype=torch.int32)
    p.kept_labels = -p.labels
    p.rep = 3 * p.labels
    p.cand_pair = torch.arange(2 * slots, dtype=torch.int32).view(slots, 2)
    p.cand_xyr = torch.arange(3 * slots, dtype=torch.float64).view(slots, 3)
    p.xy = torch.arange(2 * slots, dtype=torch.float64).view(slots, 2)
    return p, off, cnt, wi


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_whole_arrays_under_the_budget(tmp_path):
    S = 600
    p, off, cnt, wi = _pipe(S)
    bench.dump_outputs(p, S, str(tmp_path), "", 64_000_000, torch, np)
    a = _load(str(tmp_path))
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64_000_000
    assert (a["window_index"] == np.arange(S)).all() and (a["win_info"] == wi).all() and (a["seg_off"] == off).all()
    ok = [s for s in range(S) if wi[s, 3] & 0xFF == 0]
    cand = np.concatenate([off[2 * s] + np.arange(wi[s, 0]) for s in ok])
    assert (a["cand_pair"] == np.stack([2 * cand, 2 * cand + 1], 1)).all() and (a["cand_xyr"][:, 2] == 3 * cand + 2).all()
    rep = np.concatenate([off[2 * s + q] + np.arange(wi[s, 1 + q]) for s in ok for q in (0, 1)])
    assert (a["rep"] == 3 * rep).all()
    pts = np.concatenate([off[k] + np.arange(cnt[k]) for k in range(2 * S)])
    assert (a["point_slot"] == pts).all() and (a["labels"] == pts).all() and (a["kept_labels"] == -pts).all()
    assert (a["xy"] == np.stack([2 * pts, 2 * pts + 1], 1)).all()


def test_samples_are_seeded_and_in_range(tmp_path):
    S = 600
    p, off, cnt, wi = _pipe(S)
    for d in ("a", "b"):
        bench.dump_outputs(p, S, str(tmp_path / d), "", 100_000, torch, np)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= 100_000
    assert 0 < a["window_index"].size < S and (np.diff(a["window_index"]) > 0).all()
    w = a["window_index"].astype(np.int64)
    assert (a["win_info"] == wi[w]).all() and (a["seg_cnt"] == np.stack([cnt[2 * w], cnt[2 * w + 1]], 1).reshape(-1)).all()
    ps = a["point_slot"].astype(np.int64)
    seg = np.searchsorted(off, ps, side="right") - 1
    assert 0 < ps.size < cnt.sum() and ((ps >= off[seg]) & (ps < off[seg] + cnt[seg])).all()
    assert (a["labels"] == ps).all() and (a["xy"][:, 1] == 2 * ps + 1).all()
