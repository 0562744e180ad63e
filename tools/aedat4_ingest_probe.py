"""Measure the AEDAT 4 ingest (design/18_aedat4_ingest.md, design/09_measured.md): the n-event synthetic 346 x 260 stream as an AEDAT 4
file (event packets of --packet-events events, default 4096, nothing between them; every packet one LZ4 frame made once on the host —
by liblz4 through ctypes (LZ4F_compressFrame) where it can be loaded, else of stored blocks by tests/aedat4_writer.py: the JSON line
says which), then medians of --warmup + --runs runs of
  - the inflate and decode in HBM (ecal_events_from_aedat4_dev), its passes from the library's own device events (ECAL_TRACE=load)
  - the host packet index (ecal_aedat4_index_packets over the file in host memory)
  - the host-to-device copy of the same bytes from pinned memory
  - ecal_stream_create_from_aedat4_file (wall time, file in /dev/shm)
  - the host decoder EventStream::aedat42bin on the same file (--host-runs runs): one host thread inflating and decoding
  - ecal_stream_create_from_aedat_file on the AEDAT 3.1 encoding of the same events: the path this camera's files took before
and one JSON line.
usage: python tools/aedat4_ingest_probe.py [--events 50000000] [--packet-events 4096] [--warmup 5] [--runs 20] [--host-runs 3]"""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

import aedat4_writer as AW  # noqa: E402
import eventcalib_amd  # noqa: E402
import synth_stream as SS  # noqa: E402

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include "event.hpp"
int main(int argc, char **argv) {
    const auto t0 = std::chrono::steady_clock::now();
    const long long n = opengv2::EventStream::aedat42bin(argv[1]);
    std::printf("%lld %.6f\n", n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
"""
HEADER31 = b"#!AER-DAT3.1\r\n#Format: RAW\r\n#Source 1: DAVIS346\r\n#!END-HEADER\r\n"
BASE = 1_700_000_000_000_000


def liblz4_compressor():
    """bytes -> one LZ4 frame by LZ4F_compressFrame with null preferences, or None when liblz4 cannot be loaded"""
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    sz = ctypes.c_size_t
    lib.LZ4F_compressFrameBound.restype, lib.LZ4F_compressFrameBound.argtypes = sz, [sz, ctypes.c_void_p]
    lib.LZ4F_compressFrame.restype, lib.LZ4F_compressFrame.argtypes = sz, [ctypes.c_void_p, sz, ctypes.c_void_p, sz, ctypes.c_void_p]
    lib.LZ4F_isError.argtypes = [sz]
    dst = ctypes.create_string_buffer(1 << 20)

    def compress(data):
        nonlocal dst
        cap = lib.LZ4F_compressFrameBound(len(data), None)
        if cap > len(dst):
            dst = ctypes.create_string_buffer(cap)
        got = lib.LZ4F_compressFrame(dst, len(dst), data, len(data), None)
        assert not lib.LZ4F_isError(got)
        return dst.raw[:got]
    return compress


def encode4(t_us, x, y, p, per, compress):
    ev = AW.make_events(t_us, x, y, p)
    chain = []
    for a in range(0, len(ev), per):
        fb = AW.event_packet(ev[a:a + per])
        chain.append((1, compress(fb) if compress else AW.lz4_stored_frame(fb)))
    return AW.build_file(chain, AW.LZ4)


def encode31(t_us, x, y, p, per):
    body = np.stack([(x << 17) | (y << 2) | (p << 1) | 1, t_us], 1).astype("<u4")
    parts = [HEADER31]
    for a in range(0, len(body), per):
        m = min(per, len(body) - a)
        parts += [struct.pack("<hhiiiiii", 1, 1, 8, 4, 0, m, m, m), body[a:a + m].tobytes()]
    return b"".join(parts)


def median_of(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    return statistics.median(fn() for _ in range(runs))


def traced(fn, warmup, runs, pattern):
    """median of fn's wall time with the library's phase lines (stderr) gathered -> (median, {phase: median ms})"""
    trace = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)
    for _ in range(warmup):
        fn()
    sys.stderr.flush()
    os.dup2(trace.fileno(), 2)
    try:
        med = statistics.median(fn() for _ in range(runs))
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)
    trace.seek(0)
    phases = {}
    for m in re.finditer(pattern, trace.read().decode()):
        phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    return med, {k: statistics.median(v) for k, v in phases.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--packet-events", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    n = a.events
    d = tempfile.mkdtemp()
    open(os.path.join(d, "drv.cpp"), "w").write(DRIVER)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    drv = os.path.join(d, "drv")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", drv, os.path.join(d, "drv.cpp"),
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    ctx = eventcalib_amd.Context(0)
    L = ctx._L
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    t_us = torch.round(t * 1e6).to(torch.int64).cpu().numpy()
    x, y, p = (v.to(torch.int64).cpu().numpy() for v in (xy[:, 0], xy[:, 1], pol))
    del t, xy, pol
    torch.cuda.empty_cache()
    compress = liblz4_compressor()
    t0 = time.perf_counter()
    data = encode4(t_us + BASE, x, y, p, a.packet_events, compress)
    res = {"events": n, "packet_events": a.packet_events, "frames_by": "liblz4 LZ4F_compressFrame" if compress else "stored blocks",
           "file_bytes": len(data), "inflated_bytes_expected": None, "encode_s": time.perf_counter() - t0, "warmup": a.warmup, "runs": a.runs}
    host = torch.empty(len(data), dtype=torch.uint8).pin_memory()
    host.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    path4, path31 = "/dev/shm/ecal_aedat4_probe.aedat4", "/dev/shm/ecal_aedat4_probe.aedat"
    open(path4, "wb").write(data)
    open(path31, "wb").write(encode31(t_us, x, y, p, a.packet_events))
    del data, t_us, x, y, p

    def index():
        t0 = time.perf_counter()
        tab, info = ctx.aedat4_index_packets(host.numpy())
        return time.perf_counter() - t0, tab
    res["host_index_ms"] = 1e3 * median_of(lambda: index()[0], a.warmup, a.runs)
    table_np = index()[1]
    res["packets"] = len(table_np)
    table = torch.from_numpy(table_np.view("u1").copy()).cuda()
    payload = host.cuda()

    def decode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev, info = ctx.events_from_aedat4(payload, "lz4", table, capacity=n, time_base=BASE)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert info["n_events"] == n, info
        res["inflated_bytes"], res["compressed_bytes"] = info["n_inflated_bytes"], info["n_compressed_bytes"]
        return dt
    wall, phases = traced(decode, a.warmup, a.runs, r"ecal aedat4 ingest: (.+?)\s+([0-9.]+) ms")
    res["decode_wall_ms"], res["decode_phases_ms"], res["decode_device_ms"] = 1e3 * wall, phases, sum(phases.values())

    dst = torch.empty_like(payload)

    def h2d():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(host, non_blocking=True)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    res["h2d_ms"] = median_of(h2d, a.warmup, a.runs)
    del dst, payload, table, host
    torch.cuda.empty_cache()

    vp = ctypes.c_void_p

    def from_file(fn, path):
        def run():
            h = vp()
            t0 = time.perf_counter()
            rc = fn(ctx._h, path.encode(), None, ctypes.byref(h), None)
            dt = time.perf_counter() - t0
            assert rc == 0 and L.ecal_stream_size(h) == n, rc
            L.ecal_stream_destroy(h)
            return dt
        return run
    wall, phases = traced(from_file(L.ecal_stream_create_from_aedat4_file, path4), a.warmup, a.runs,
                          r"ecal aedat4 ingest: (host packet index|file read \+ upload|index beside upload)\s+([0-9.]+) ms")
    res["stream_from_aedat4_file_s"], res["file_phases_ms"] = wall, phases
    res["stream_from_aedat31_file_s"] = traced(from_file(L.ecal_stream_create_from_aedat_file, path31), a.warmup, a.runs, r"(x)(y)")[0]
    host_s = []
    for _ in range(a.host_runs):
        out = subprocess.run([drv, path4], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == n
        host_s.append(float(out[1]))
    res["host_aedat42bin_s"], res["host_aedat42bin_runs"] = (statistics.median(host_s) if host_s else None), host_s
    for f in (path4, path31, path4[:-7] + ".bin"):
        if os.path.exists(f):
            os.remove(f)
    del res["inflated_bytes_expected"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
