"""Measure the AEDAT ingest (design/15_aedat_ingest.md, design/09_measured.md): the n-event synthetic 346 x 260 stream encoded as AEDAT
3.1 (polarity packets of --packet-events events, default 4096, nothing between them) and as AEDAT 2.0 (one record per event), then
per format medians of --warmup + --runs runs of
  - the decode in HBM (ecal_events_from_aedat_dev), its passes from the library's own device events (ECAL_TRACE=load)
  - 3.1: the host packet index (ecal_aedat_index_packets over the payload in host memory; and over the file's headers alone, the
    "host packet index" line of the file form)
  - the host-to-device copy of the same bytes from pinned memory
  - ecal_stream_create_from_aedat_file (wall time, file in /dev/shm)
  - the host decoder EventStream::aedat2bin on the same file (--host-runs runs)
and one JSON line per format.
usage: python tools/aedat_ingest_probe.py [--events 50000000] [--packet-events 4096] [--warmup 5] [--runs 20] [--host-runs 3]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import struct
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
    const long long n = opengv2::EventStream::aedat2bin(argv[1]);
    std::printf("%lld %.6f\n", n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
"""
HEADERS = {"3.1": b"#!AER-DAT3.1\r\n#Format: RAW\r\n#Source 1: DAVIS346\r\n#!END-HEADER\r\n", "2.0": b"#!AER-DAT2.0\r\n# AER data\r\n"}


def as_bytes(words, big_endian):
    """int64 values below 2^32 as their 32-bit words' bytes (a uint8 tensor)"""
    b = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32).view(torch.uint8).reshape(-1, 4)
    return (b.flip(1) if big_endian else b).reshape(-1)


def encode(fmt, t_us, x, y, p, per):
    """the events as payload bytes (a uint8 CUDA tensor)"""
    n = t_us.numel()
    if fmt == "2.0":
        return as_bytes(torch.stack([(y << 22) | (x << 12) | (p << 11), t_us & 0xFFFFFFFF], 1).reshape(-1), True)
    assert int(t_us.max()) < 1 << 31                  # (one overflow value for the whole stream: 35 minutes)
    body = as_bytes(torch.stack([(x << 17) | (y << 2) | (p << 1) | 1, t_us], 1).reshape(-1), False)
    parts = []
    n_full = n // per
    if n_full:
        head = torch.frombuffer(bytearray(struct.pack("<hhiiiiii", 1, 1, 8, 4, 0, per, per, per)), dtype=torch.uint8).to(body.device)
        parts.append(torch.cat([head.expand(n_full, 28), body[: n_full * per * 8].view(n_full, per * 8)], 1).reshape(-1))
    if n % per:
        m = n % per
        parts += [torch.frombuffer(bytearray(struct.pack("<hhiiiiii", 1, 1, 8, 4, 0, m, m, m)), dtype=torch.uint8).to(body.device), body[n_full * per * 8:]]
    return torch.cat(parts)


def median_of(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    return statistics.median(fn() for _ in range(runs))


def probe(ctx, fmt, n, a, drv):
    L = ctx._L
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    t_us = torch.round(t * 1e6).to(torch.int64)
    payload = encode(fmt, t_us, xy[:, 0].to(torch.int64), xy[:, 1].to(torch.int64), pol.to(torch.int64), a.packet_events)
    del t, xy, pol, t_us
    torch.cuda.empty_cache()
    res = {"format": fmt, "events": n, "payload_bytes": payload.numel(), "warmup": a.warmup, "runs": a.runs}
    host = torch.empty(payload.numel(), dtype=torch.uint8).pin_memory()
    host.copy_(payload)

    # ---- 3.1: the packet index over the payload in host memory
    table = None
    if fmt == "3.1":
        res["packet_events"] = a.packet_events

        def index():
            t0 = time.perf_counter()
            tab, info = ctx.aedat_index_packets(host.numpy())
            dt = time.perf_counter() - t0
            assert info["n_raw_events"] == n
            return dt, tab
        res["host_index_ms"] = 1e3 * median_of(lambda: index()[0], a.warmup, a.runs)
        table_np = index()[1]
        res["packets"] = len(table_np)
        table = torch.from_numpy(table_np.view("u1").copy()).cuda()

    # ---- the decode in HBM; the library's phase lines (stderr) into a file
    trace = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)

    def decode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev, info = ctx.events_from_aedat(payload, fmt, packets=table, capacity=n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert info["n_events"] == n and info["n_invalid"] == 0, info
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
    for m in re.finditer(r"ecal aedat ingest: (.+?)\s+([0-9.]+) ms", trace.read().decode()):
        phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    res["decode_phases_ms"] = {k: statistics.median(v) for k, v in phases.items()}
    res["decode_device_ms"] = sum(res["decode_phases_ms"].values())

    # ---- the upload of the same bytes
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
    path = "/dev/shm/ecal_aedat_probe.aedat"
    with open(path, "wb") as f:
        f.write(HEADERS[fmt])
        host.numpy().tofile(f)
    del host, payload, table
    torch.cuda.empty_cache()
    vp = ctypes.c_void_p

    def from_file():
        h = vp()
        t0 = time.perf_counter()
        rc = L.ecal_stream_create_from_aedat_file(ctx._h, path.encode(), None, ctypes.byref(h), None)
        dt = time.perf_counter() - t0
        assert rc == 0 and L.ecal_stream_size(h) == n, rc
        L.ecal_stream_destroy(h)
        return dt
    trace2 = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    os.dup2(trace2.fileno(), 2)
    try:
        res["stream_from_aedat_file_s"] = median_of(from_file, a.warmup, a.runs)
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
    trace2.seek(0)
    file_phases = {}
    for m in re.finditer(r"ecal aedat ingest: (host packet index|file read \+ upload|index beside upload)\s+([0-9.]+) ms", trace2.read().decode()):
        file_phases.setdefault(m.group(1), []).append(float(m.group(2)))
    res["file_phases_ms"] = {k: statistics.median(v[a.warmup:] or v) for k, v in file_phases.items()}
    host_s = []
    for _ in range(a.host_runs):
        out = subprocess.run([drv, path], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == n
        host_s.append(float(out[1]))
    res["host_aedat2bin_s"], res["host_aedat2bin_runs"] = (statistics.median(host_s) if host_s else None), host_s
    for f in (path, path[:-6] + ".bin"):
        if os.path.exists(f):
            os.remove(f)
    os.close(saved)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--packet-events", type=int, default=4096)
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
    for fmt in ("3.1", "2.0"):
        probe(ctx, fmt, a.events, a, drv)


if __name__ == "__main__":
    main()
