"""Measure the raw ingest (design/13_raw_ingest.md, design/09_measured.md): the n-event synthetic stream encoded as EVT3 and as EVT2
(a state word wherever time high, time low or the row changes, one ADDR_X / CD word per event), then per format medians of
--warmup + --runs runs of
  - the decode in HBM (ecal_events_from_raw_dev), its passes from the library's own device events (ECAL_TRACE=load)
  - the host-to-device copy of the same bytes from pinned memory
  - ecal_stream_create_from_raw_file (wall time, file in /dev/shm)
  - the host decoder EventStream::raw2bin on the same file (--host-runs runs)
and one JSON line per format.   usage: python tools/raw_ingest_probe.py [--events 50000000] [--warmup 5] [--runs 20] [--host-runs 3]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ECAL_TRACE"] = "load"
import torch  # noqa: E402

import eventcalib_amd  # noqa: E402
import synth_stream as SS  # noqa: E402

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include "event.hpp"
int main(int argc, char **argv) {
    const auto t0 = std::chrono::steady_clock::now();
    const long long n = opengv2::EventStream::raw2bin(argv[1]);
    std::printf("%lld %.6f\n", n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
"""


def encode(fmt, t_us, x, y, p):
    """the events as payload bytes (a uint8 CUDA tensor): TIME_HIGH / TIME_LOW / ADDR_Y where they change, then the event's word"""
    n = t_us.numel()

    def changed(v):
        c = torch.ones(n, dtype=torch.bool, device=v.device)
        c[1:] = v[1:] != v[:-1]
        return c
    if fmt == "EVT3":
        parts = [(changed((t_us >> 12) & 0xFFF), (0x8 << 12) | ((t_us >> 12) & 0xFFF)), (changed(t_us & 0xFFF), (0x6 << 12) | (t_us & 0xFFF)),
                 (changed(y), y), (torch.ones(n, dtype=torch.bool, device=x.device), (0x2 << 12) | (p << 11) | x)]
    else:
        parts = [(changed(t_us >> 6), (0x8 << 28) | (t_us >> 6)),
                 (torch.ones(n, dtype=torch.bool, device=x.device), (p << 28) | ((t_us & 0x3F) << 22) | (x << 11) | y)]
    count = sum(m.to(torch.int64) for m, _ in parts)
    at = torch.cumsum(count, 0) - count
    out = torch.zeros(int(count.sum()), dtype=torch.int64, device=x.device)
    for m, w in parts:
        out[at[m]] = w[m]
        at = at + m
    if fmt == "EVT3":
        return torch.where(out >= 1 << 15, out - (1 << 16), out).to(torch.int16).view(torch.uint8).reshape(-1)   # (the same 16 bits)
    return torch.where(out >= 1 << 31, out - (1 << 32), out).to(torch.int32).view(torch.uint8).reshape(-1)


def median_of(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    return statistics.median(fn() for _ in range(runs))


def probe(ctx, fmt, n, a, drv):
    L = ctx._L
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    t_us = torch.round(t * 1e6).to(torch.int64)
    payload = encode(fmt, t_us, xy[:, 0].to(torch.int64), xy[:, 1].to(torch.int64), pol.to(torch.int64))
    del t, xy, pol, t_us
    torch.cuda.empty_cache()
    res = {"format": fmt, "events": n, "payload_bytes": payload.numel(), "warmup": a.warmup, "runs": a.runs}

    # ---- the decode in HBM; the library's phase lines (stderr) into a file
    trace = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)

    def decode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev, info = ctx.events_from_raw(payload, fmt, capacity=n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert info["n_events"] == n and info["n_no_state"] == 0, info
        return dt
    for _ in range(a.warmup):
        decode()
    sys.stderr.flush()
    os.dup2(trace.fileno(), 2)
    try:
        res["decode_wall_ms"] = 1e3 * statistics.median(decode() for _ in range(a.runs))
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
    trace.seek(0)
    phases = {}
    for m in re.finditer(r"ecal raw ingest: (.+?)\s+([0-9.]+) ms", trace.read().decode()):
        phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    res["decode_phases_ms"] = {k: statistics.median(v) for k, v in phases.items()}
    res["decode_device_ms"] = sum(res["decode_phases_ms"].values())

    # ---- the upload of the same bytes
    host = torch.empty(payload.numel(), dtype=torch.uint8).pin_memory()
    host.copy_(payload)
    dst = torch.empty_like(payload)

    def h2d():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(host, non_blocking=True)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    res["h2d_ms"] = median_of(h2d, a.warmup, a.runs)
    del dst

    # ---- the file forms
    raw = "/dev/shm/ecal_raw_probe.raw"
    with open(raw, "wb") as f:
        f.write(b"% evt 3.0\n% end\n" if fmt == "EVT3" else b"% evt 2.0\n% end\n")
        host.numpy().tofile(f)
    del host, payload
    torch.cuda.empty_cache()
    vp = ctypes.c_void_p

    def from_raw_file():
        h = vp()
        t0 = time.perf_counter()
        rc = L.ecal_stream_create_from_raw_file(ctx._h, raw.encode(), None, ctypes.byref(h), None)
        dt = time.perf_counter() - t0
        assert rc == 0 and L.ecal_stream_size(h) == n, rc
        L.ecal_stream_destroy(h)
        return dt
    os.dup2(trace.fileno(), 2)      # (the phase lines of these runs are not wanted)
    try:
        res["stream_from_raw_file_s"] = median_of(from_raw_file, a.warmup, a.runs)
    finally:
        os.dup2(saved, 2)
    host_s = []
    for _ in range(a.host_runs):
        out = subprocess.run([drv, raw], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == n
        host_s.append(float(out[1]))
    res["host_raw2bin_s"], res["host_raw2bin_runs"] = (statistics.median(host_s) if host_s else None), host_s
    for path in (raw, raw[:-4] + ".bin"):
        if os.path.exists(path):
            os.remove(path)
    os.close(saved)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    open(os.path.join(d, "drv.cpp"), "w").write(DRIVER)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    drv = os.path.join(d, "drv")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", drv, os.path.join(d, "drv.cpp"),
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    ctx = eventcalib_amd.Context(0)
    for fmt in ("EVT3", "EVT2"):
        probe(ctx, fmt, a.events, a, drv)


if __name__ == "__main__":
    main()
