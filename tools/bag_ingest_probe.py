"""Measure the bag ingest (design/16_bag_ingest.md, design/09_measured.md): the n-event synthetic 346 x 260 stream written as a ROS 1
bag (format 2.0: dvs_msgs/EventArray messages of --message-events events, default 4096, --chunk-messages of them a chunk, default 14,
nothing between them), then medians of --warmup + --runs runs of
  - the decode in HBM (ecal_events_from_bag_dev), its passes from the library's own device events (ECAL_TRACE=load)
  - the host message index (ecal_bag_index_messages over the file in host memory; and over the file's record headers, the "host
    message index" line of the file form)
  - the host-to-device copy of the same bytes from pinned memory
  - ecal_stream_create_from_bag_file (wall time, file in /dev/shm)
  - the host decoder EventStream::bag2bin on the same file (--host-runs runs)
and one JSON line.
usage: python tools/bag_ingest_probe.py [--events 50000000] [--message-events 4096] [--chunk-messages 14] [--warmup 5] [--runs 20] [--host-runs 3]"""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bag_writer as bw  # noqa: E402
import eventcalib_amd  # noqa: E402
import synth_stream as SS  # noqa: E402

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include "event.hpp"
int main(int argc, char **argv) {
    const auto t0 = std::chrono::steady_clock::now();
    const long long n = opengv2::EventStream::bag2bin(argv[1]);
    std::printf("%lld %.6f\n", n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
"""
BASE = 1600000000 * 10 ** 9
CONN = (0, "/dvs/events", bw.DVS)
FRAME_ID = b"davis"


def dev_bytes(b, device):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(device)


def encode(t_ns, x, y, p, per, cm):
    """the events as the bytes of a bag (a uint8 CUDA tensor): a chunk with the connection record, chunks of cm messages of per events,
    a last chunk with the rest, the connection again behind them"""
    n, dev = t_ns.numel(), t_ns.device
    ev = torch.empty(n, 13, dtype=torch.uint8, device=dev)
    ev[:, 0:2] = x.to(torch.int16).view(torch.uint8).reshape(n, 2)
    ev[:, 2:4] = y.to(torch.int16).view(torch.uint8).reshape(n, 2)
    ev[:, 4:8] = (t_ns // 10 ** 9).to(torch.int32).view(torch.uint8).reshape(n, 4)
    ev[:, 8:12] = (t_ns % 10 ** 9).to(torch.int32).view(torch.uint8).reshape(n, 4)
    ev[:, 12] = p.to(torch.uint8)
    empty = np.zeros(per, bw.EVENT_DTYPE)
    front = bw.message_record(0, bw.event_array_message(empty, frame_id=FRAME_ID))[: -13 * per]      # record header + the message's 28 + L bytes
    msg_bytes = len(front) + 13 * per
    n_chunks = n // (per * cm)
    parts = [dev_bytes(bw.MAGIC + bw.bag_header_record(0, 1, n_chunks + 2) + bw.chunk_record(bw.connection_record(*CONN)), dev)]
    if n_chunks:
        chunk_front = bw.chunk_record(b"\0" * (cm * msg_bytes))[: -cm * msg_bytes]
        body = ev[: n_chunks * cm * per].view(n_chunks * cm, per * 13)
        msgs = torch.cat([dev_bytes(front, dev).expand(n_chunks * cm, len(front)), body], 1).view(n_chunks, cm * msg_bytes)
        parts.append(torch.cat([dev_bytes(chunk_front, dev).expand(n_chunks, len(chunk_front)), msgs], 1).reshape(-1))
    rest = ev[n_chunks * cm * per:].cpu().numpy().view(bw.EVENT_DTYPE).reshape(-1)
    inner = b"".join(bw.message_record(0, bw.event_array_message(rest[a: a + per], frame_id=FRAME_ID)) for a in range(0, len(rest), per))
    parts.append(dev_bytes((bw.chunk_record(inner) if inner else b"") + bw.connection_record(*CONN), dev))
    return torch.cat(parts)


def median_of(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    return statistics.median(fn() for _ in range(runs))


def probe(ctx, n, a, drv):
    L = ctx._L
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    t_ns = torch.round(t * 1e9).to(torch.int64) + BASE
    base = int(t_ns[0]) // 10 ** 9 * 10 ** 9
    payload = encode(t_ns, xy[:, 0].to(torch.int64), xy[:, 1].to(torch.int64), pol.to(torch.int64), a.message_events, a.chunk_messages)
    del t, xy, pol, t_ns
    torch.cuda.empty_cache()
    res = {"events": n, "file_bytes": payload.numel(), "message_events": a.message_events, "chunk_messages": a.chunk_messages, "warmup": a.warmup,
           "runs": a.runs}
    host = torch.empty(payload.numel(), dtype=torch.uint8).pin_memory()
    host.copy_(payload)

    # ---- the message index over the file in host memory (one walk: the capacity is known)
    n_messages = (n + a.message_events - 1) // a.message_events

    def index():
        t0 = time.perf_counter()
        tab, info = ctx.bag_index_messages(host.numpy(), capacity=n_messages)
        dt = time.perf_counter() - t0
        assert info["n_raw_events"] == n and info["first_stamp_ns"] == base, info
        return dt, tab
    res["host_index_ms"] = 1e3 * median_of(lambda: index()[0], a.warmup, a.runs)
    table_np = index()[1]
    res["messages"] = len(table_np)
    table = torch.from_numpy(table_np.view("u1").copy()).cuda()

    # ---- the decode in HBM; the library's phase lines (stderr) into a file
    trace = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)

    def decode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev, info = ctx.events_from_bag(payload, table, capacity=n, time_base=base)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert info["n_events"] == n, info
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
    for m in re.finditer(r"ecal bag ingest: (.+?)\s+([0-9.]+) ms", trace.read().decode()):
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
    path = "/dev/shm/ecal_bag_probe.bag"
    with open(path, "wb") as f:
        host.numpy().tofile(f)
    del host, payload, table
    torch.cuda.empty_cache()
    vp = ctypes.c_void_p

    def from_file():
        h = vp()
        t0 = time.perf_counter()
        rc = L.ecal_stream_create_from_bag_file(ctx._h, path.encode(), None, ctypes.byref(h), None)
        dt = time.perf_counter() - t0
        assert rc == 0 and L.ecal_stream_size(h) == n, rc
        L.ecal_stream_destroy(h)
        return dt
    trace2 = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    os.dup2(trace2.fileno(), 2)
    try:
        res["stream_from_bag_file_s"] = median_of(from_file, a.warmup, a.runs)
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
    trace2.seek(0)
    file_phases = {}
    for m in re.finditer(r"ecal bag ingest: (host message index|file read \+ upload|index beside upload)\s+([0-9.]+) ms", trace2.read().decode()):
        file_phases.setdefault(m.group(1), []).append(float(m.group(2)))
    res["file_phases_ms"] = {k: statistics.median(v[a.warmup:] or v) for k, v in file_phases.items()}
    host_s = []
    for _ in range(a.host_runs):
        out = subprocess.run([drv, path], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == n
        host_s.append(float(out[1]))
    res["host_bag2bin_s"], res["host_bag2bin_runs"] = (statistics.median(host_s) if host_s else None), host_s
    for f in (path, path[:-4] + ".bin"):
        if os.path.exists(f):
            os.remove(f)
    os.close(saved)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--message-events", type=int, default=4096)
    ap.add_argument("--chunk-messages", type=int, default=14)
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
    probe(ctx, a.events, a, drv)


if __name__ == "__main__":
    main()
