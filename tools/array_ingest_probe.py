"""Measure the array ingest (design/21_array_ingest.md, design/09_measured.md): the n-event synthetic 346 x 260 stream held as the common
column layout — int64 t (microseconds), uint16 x, uint16 y, uint8 p, natural strides, 13 bytes an event — then, in ONE run, medians and
spreads of --warmup + --runs runs of
  - ecal_events_from_fields_dev on those columns in HBM: the whole call between two HIP events, and its passes from the library's own
    device events (ECAL_TRACE=load)
  - (a) ecal_events_from_bag_dev on the same events as a bag (tools/bag_ingest_probe.py's encoder): the other ingest that reads 13 bytes
    an event twice and writes 25 once
  - (b) the host-to-device copy of the columns' bytes from pinned memory
  - (c) on the host, what a user does without this call: numpy packing the structured 25-byte array from the four columns, at
    --host-events events, scaled to n
  - ecal_stream_create_from_fields on the columns in host memory and ecal_stream_create_from_npy_file on the same events as a .npy of
    packed 13-byte items in /dev/shm (wall time, two warm-up runs and runs / 4 timed ones)
  - ecal_events_to_fields_dev (the records back into the same column types) against ecal_filter_events_dev with everything kept: the
    other pass that reads every record once and writes it out again
and one JSON line.
usage: python tools/array_ingest_probe.py [--events 50000000] [--host-events 5000000] [--warmup 5] [--runs 20]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["ECAL_TRACE"] = "load"
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eventcalib_amd  # noqa: E402
import synth_stream as SS  # noqa: E402
from bag_ingest_probe import encode  # noqa: E402
from eventcalib_amd import capi  # noqa: E402

BASE_US = 1600000000 * 10 ** 6
RECORD = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "spread_ms": ms[-1] - ms[0]}


def timed(fn, warmup, runs):
    """device time of fn between two HIP events on the current stream, per run"""
    out = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


class Trace:
    """the library's phase lines (stderr) of the calls inside the block, by phase name"""
    def __init__(self, tag):
        self.tag, self.phases = tag, {}

    def __enter__(self):
        self.file, self.saved = tempfile.TemporaryFile(mode="w+b"), os.dup(2)
        sys.stderr.flush()
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        for m in re.finditer(r"ecal %s ingest: (.+?)\s+([0-9.]+) ms" % re.escape(self.tag), self.file.read().decode()):
            self.phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))

    def medians(self, runs):
        return {k: statistics.median(v[-runs:]) for k, v in self.phases.items()}


def probe(ctx, n, a):
    stream = torch.cuda.current_stream().cuda_stream
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    t_us = torch.round(t * 1e6).to(torch.int64) + BASE_US
    base = int(t_us[0]) // 10 ** 6 * 10 ** 6
    x16, y16, p8 = xy[:, 0].to(torch.int16).contiguous(), xy[:, 1].to(torch.int16).contiguous(), pol.to(torch.uint8).contiguous()
    del t, xy, pol
    res = {"events": n, "column_bytes": 13 * n, "warmup": a.warmup, "runs": a.runs}

    # ---- the array ingest on the columns in HBM
    f = (capi.Field * 4)(capi.Field(t_us.data_ptr(), 8, capi.field_type(np.int64), 0), capi.Field(x16.data_ptr(), 2, capi.field_type(np.uint16), 0),
                         capi.Field(y16.data_ptr(), 2, capi.field_type(np.uint16), 0), capi.Field(p8.data_ptr(), 1, capi.field_type(np.uint8), 0))
    opt = capi.fields_options(time_magnitude=1e-6, time_base=base)
    records = torch.empty(n * 25 + 16, dtype=torch.uint8, device="cuda")

    def pack():
        info = ctx.events_from_fields_dev(f, n, opt, records.data_ptr(), n, stream)
        assert info["n_events"] == n, info
    with Trace("array") as tr:
        res["from_fields"] = stats(timed(pack, a.warmup, a.runs))
    res["from_fields"]["phases_ms"] = tr.medians(a.runs)

    # ---- (a) the bag ingest on the same events
    payload = encode(t_us * 1000, x16.to(torch.int64), y16.to(torch.int64), p8.to(torch.int64), 4096, 14)
    host_file = payload.cpu().numpy()
    table_np, _ = ctx.bag_index_messages(host_file)
    table = torch.from_numpy(table_np.view("u1").copy()).cuda()
    mt, n_m = ctx._table_tensor(table, capi.BAG_MESSAGE_DTYPE, payload.device)
    bopt = ctx.bag_options(time_base=base * 1000)
    L = ctx._L
    bag_records = torch.empty(n * 25 + 16, dtype=torch.uint8, device="cuda")

    def bag():
        info = capi.BagInfo()
        rc = L.ecal_events_from_bag_dev(ctx._h, payload.data_ptr(), payload.numel(), mt.data_ptr(), n_m, ctypes.byref(bopt), bag_records.data_ptr(), n,
                                        ctypes.byref(info), stream)
        assert rc == 0 and info.n_events == n, (rc, info.n_events)
    ctx.events_from_bag(payload, table, capacity=n, time_base=base * 1000)   # (a first warm run)
    with Trace("bag") as tr:
        res["from_bag"] = stats(timed(bag, a.warmup, a.runs))
    res["from_bag"]["phases_ms"] = tr.medians(a.runs)
    res["same_records"] = bool(torch.equal(records[: n * 25].view(-1, 25)[:, 8:], bag_records[: n * 25].view(-1, 25)[:, 8:]))   # (x, y, p: the stamps differ in the last bit by the tick)
    res["ratio_to_bag"] = res["from_fields"]["median_ms"] / res["from_bag"]["median_ms"]
    del payload, table, mt, bag_records, host_file
    torch.cuda.empty_cache()

    # ---- (b) the upload of the columns' bytes
    host = torch.empty(13 * n, dtype=torch.uint8).pin_memory()
    dst = torch.empty(13 * n, dtype=torch.uint8, device="cuda")
    res["h2d"] = stats(timed(lambda: dst.copy_(host, non_blocking=True), a.warmup, a.runs))
    del host, dst

    # ---- (c) the host detour: numpy packs the 25-byte records from the columns
    m = min(n, a.host_events)
    ht, hx, hy, hp = t_us[:m].cpu().numpy(), x16[:m].cpu().numpy().view(np.uint16), y16[:m].cpu().numpy().view(np.uint16), p8[:m].cpu().numpy()
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        rec = np.empty(m, RECORD)
        rec["t"] = (ht - base).astype(np.float64) * 1e-6
        rec["x"], rec["y"], rec["p"] = hx, hy, hp
        host_s.append(time.perf_counter() - t0)
    res["host_pack"] = {"events": m, "median_s": statistics.median(host_s), "scaled_to_n_s": statistics.median(host_s) * n / m}
    assert rec.tobytes() == records[: m * 25].cpu().numpy().tobytes()
    del rec

    # ---- the stream forms (wall time): HOST columns, and the same events as a .npy of packed 13-byte items in /dev/shm
    vp = ctypes.c_void_p
    hcols = [capi._host_column(c) for c in (t_us.cpu().numpy(), x16.cpu().numpy().view(np.uint16), y16.cpu().numpy().view(np.uint16), p8.cpu().numpy())]
    hf = (capi.Field * 4)(*[c[1] for c in hcols])

    def wall(call):
        h = vp()
        t0 = time.perf_counter()
        rc = call(h)
        dt = time.perf_counter() - t0
        assert rc == 0 and L.ecal_stream_size(h) == n, rc
        L.ecal_stream_destroy(h)
        return dt
    host_runs = max(3, a.runs // 4)
    with Trace("array"):
        s = [wall(lambda h: L.ecal_stream_create_from_fields(ctx._h, hf, n, ctypes.byref(opt), ctypes.byref(h), None)) for _ in range(2 + host_runs)][2:]
    res["stream_from_host_columns_s"] = {"median_s": statistics.median(s), "runs": s}
    arr = np.empty(n, np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")]))
    for name, c in zip("txyp", hcols):
        arr[name] = c[0]
    path = "/dev/shm/ecal_array_probe.npy"
    np.save(path, arr)
    del arr
    nopt = capi.npy_options(time_magnitude=1e-6, time_base=base)
    try:
        with Trace("array"):
            s = [wall(lambda h: L.ecal_stream_create_from_npy_file(ctx._h, path.encode(), ctypes.byref(nopt), ctypes.byref(h), None)) for _ in range(2 + host_runs)][2:]
    finally:
        os.remove(path)
    res["stream_from_npy_file_s"] = {"median_s": statistics.median(s), "runs": s}
    del hcols, hf

    # ---- the reverse against the filter with everything kept
    out = [torch.empty_like(t_us), torch.empty_like(x16), torch.empty_like(y16), torch.empty_like(p8)]
    g = (capi.Field * 4)(*[capi.Field(o.data_ptr(), f[k].stride, f[k].type, 0) for k, o in enumerate(out)])
    topt = capi.to_fields_options(time_base=base)

    def unpack():
        info = ctx.events_to_fields_dev(records.data_ptr(), n, g, topt, stream)
        assert info["n_unrepresentable"] == 0
    with Trace("array export") as tr:
        res["to_fields"] = stats(timed(unpack, a.warmup, a.runs))
    res["to_fields"]["phases_ms"] = tr.medians(a.runs)
    res["round_trip_exact"] = bool(torch.equal(out[0], t_us) and torch.equal(out[1], x16) and torch.equal(out[2], y16) and torch.equal(out[3], p8))
    del out
    mask = torch.zeros(260 * 346, dtype=torch.uint8, device="cuda")
    kept = torch.empty(n * 25 + 16, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")

    def keep_all():
        ctx.filter_events_dev(records.data_ptr(), n, mask.data_ptr(), 346, 260, kept.data_ptr(), count.data_ptr(), None, stream)
    res["filter_keep_all"] = stats(timed(keep_all, a.warmup, a.runs))
    assert int(count.item()) == n
    res["ratio_to_filter"] = res["to_fields"]["median_ms"] / res["filter_keep_all"]["median_ms"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--host-events", type=int, default=5_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    ctx = eventcalib_amd.Context(0)
    probe(ctx, a.events, a)


if __name__ == "__main__":
    main()
