"""Measure the text ingest (design/12_text_ingest.md, design/09_measured.md): an n-line text of "stamp x y polarity" lines made from
the synthetic stream, then medians of --warmup + --runs runs of
  - the parse in HBM (ecal_events_from_text_dev), its phases from the library's own device events (ECAL_TRACE=load)
  - the host-to-device copy of the same bytes from pinned memory
  - ecal_stream_create_from_text_file (wall time, file in /dev/shm)
  - the host converter EventStream::txt2bin on the same file (--host-runs runs: it takes tens of seconds)
  - ecal_stream_create_from_file on the .bin it wrote
and one JSON line.   usage: python tools/text_ingest_probe.py [--lines 50000000] [--warmup 5] [--runs 20] [--host-runs 3]"""
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
    const long long n = opengv2::EventStream::txt2bin(argv[1], 1e-6, 0);
    std::printf("%lld %.6f\n", n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
"""


def make_text(n):
    """"%10d %3d %3d %d\n" per event of the synthetic stream (blank-padded fields: 21 bytes a line), on the GPU"""
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    out = torch.full((n, 21), 32, dtype=torch.uint8, device="cuda")

    def put(col, width, v):
        v = v.to(torch.int64)
        for k in range(width):
            d = (v // 10 ** k) % 10
            shown = (v >= 10 ** k) | (k == 0)
            out[:, col + width - 1 - k] = torch.where(shown, d + 48, torch.full_like(d, 32)).to(torch.uint8)
    put(0, 10, torch.round(t * 1e6))
    put(11, 3, xy[:, 0])
    put(15, 3, xy[:, 1])
    out[:, 19] = pol + 48
    out[:, 20] = 10
    return out.reshape(-1)


def median_of(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    return statistics.median(fn() for _ in range(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=50_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    n = a.lines
    text = make_text(n)
    res = {"lines": n, "text_bytes": text.numel(), "warmup": a.warmup, "runs": a.runs}
    ctx = eventcalib_amd.Context(0)
    L = ctx._L

    # ---- the parse in HBM; the library's phase lines (stderr) into a file
    trace = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)

    def parse():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev, info = ctx.events_from_text(text, capacity=n + 1, time_base=0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert info["n_events"] == n + 1 and info["n_host_lines"] == 0, info
        return dt
    for _ in range(a.warmup):
        parse()
    sys.stderr.flush()
    os.dup2(trace.fileno(), 2)
    try:
        res["parse_wall_ms"] = 1e3 * statistics.median(parse() for _ in range(a.runs))
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
    trace.seek(0)
    phases = {}
    for m in re.finditer(r"ecal text ingest: (.+?)\s+([0-9.]+) ms", trace.read().decode()):
        phases.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    res["parse_phases_ms"] = {k: statistics.median(v) for k, v in phases.items()}
    res["parse_phases_runs"] = {k: len(v) for k, v in phases.items()}

    # ---- the upload of the same bytes
    host = torch.empty(text.numel(), dtype=torch.uint8).pin_memory()
    host.copy_(text)
    dst = torch.empty_like(text)

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
    txt = "/dev/shm/ecal_text_probe.txt"
    host.numpy().tofile(txt)
    del host, text
    torch.cuda.empty_cache()
    vp = ctypes.c_void_p
    opt = ctx.text_options(time_base=0)

    def from_text_file():
        h = vp()
        t0 = time.perf_counter()
        rc = L.ecal_stream_create_from_text_file(ctx._h, txt.encode(), ctypes.byref(opt), ctypes.byref(h), None)
        dt = time.perf_counter() - t0
        assert rc == 0 and L.ecal_stream_size(h) == n + 1, rc
        L.ecal_stream_destroy(h)
        return dt
    os.dup2(trace.fileno(), 2)      # (the phase lines of these runs are not wanted)
    try:
        res["stream_from_text_file_s"] = median_of(from_text_file, a.warmup, a.runs)
    finally:
        os.dup2(saved, 2)

    d = tempfile.mkdtemp()
    open(os.path.join(d, "drv.cpp"), "w").write(DRIVER)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", os.path.join(d, "drv"),
                           os.path.join(d, "drv.cpp"), "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    host_s = []
    for _ in range(a.host_runs):
        out = subprocess.run([os.path.join(d, "drv"), txt], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == n + 1
        host_s.append(float(out[1]))
    res["host_txt2bin_s"], res["host_txt2bin_runs"] = (statistics.median(host_s) if host_s else None), host_s
    binf = txt[:-4] + ".bin"
    if host_s:
        def from_bin_file():
            h = vp()
            t0 = time.perf_counter()
            rc = L.ecal_stream_create_from_file(ctx._h, binf.encode(), 0.0, 0, 0.0, ctypes.byref(h))
            dt = time.perf_counter() - t0
            assert rc == 0 and L.ecal_stream_size(h) == n + 1, rc
            L.ecal_stream_destroy(h)
            return dt
        os.dup2(trace.fileno(), 2)
        try:
            res["stream_from_bin_file_s"] = median_of(from_bin_file, a.warmup, a.runs)
        finally:
            os.dup2(saved, 2)
        os.remove(binf)
    os.remove(txt)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
